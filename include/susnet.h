/*
 * susnet.h -- C ABI of libsusnet_hip.so: batched, MI355X-native (gfx950) implementation of the Sus-Net
 * grid-world environment hot path (reset / sample_actions / step / fused random rollout / observation
 * extraction), stepping `batch` independent episodes in lockstep, one wavefront lane per environment.
 *
 * The reference is a pure-Python gymnasium.Env (no FFI of its own), so every entry point names the
 * reference METHOD it replaces (paths relative to the reference repo root):
 *
 *   susnet_create          FourRoomEnv.__init__            src/environment/base.py:103-228
 *                          ImposterTrainingGround.__init__ src/environment/pred_prey.py:26-76
 *                          FourRoomEnvWithTagging.__init__ src/environment/tagging.py:10-60
 *   susnet_reset           FourRoomEnv.reset               src/environment/base.py:251-324 (tagging.py:62-101)
 *   susnet_sample_actions  FourRoomEnv.sample_actions      src/environment/base.py:326-330
 *   susnet_policy_actions  run_game's acting step          src/visualize.py:547-562 (train.py:355-381, epsilon = 0)
 *   susnet_agent_policy_actions  train()'s acting step with one Q row per agent  src/train.py:351-381 (SpatialDQN on each agent's view)
 *   susnet_qnet_*          MLP.forward on the flat features src/models/dqn.py:72-108, 322-329
 *   susnet_mlp_forward     MLP.forward of any served layer stack on caller-supplied feature rows  src/models/dqn.py:72-108, 322-329
 *   susnet_spatial_forward SpatialDQN.forward (eval mode) on the planes / perspective features     src/models/dqn.py:141-301
 *   susnet_spatial_forward_dropout  the same in training mode: nn.RNN's dropout between layers, as the trainer's agents act  src/train.py:104, 355-381
 *   susnet_window_push     the acting loop's state window, one tick on (as feature rows)  src/train.py:318-322, 388-389, 441-445
 *   susnet_state_window_push  the acting loop's RAW state window [B][T][S] uint8, one tick on, in place  src/train.py:388-389, 441-445
 *   susnet_policy_step     argmax per team + env.step        src/visualize.py:547-582
 *   susnet_step            FourRoomEnv.step                src/environment/base.py:332-407 (tagging.py:120-235)
 *                          + _agent_step 462-533, check_win_condition 409-460 (pred_prey.py:78-99),
 *                            _merge_rewards 553-563, EnvMetricHandler src/metrics.py:35-64
 *   susnet_rollout         ReplayBuffer.populate's loop    src/replay_memory.py:96-143 (minus the buffer)
 *   susnet_ring_append     ReplayBuffer.add x (T x B)      src/replay_memory.py:50-73, with populate's sequence window (108-136)
 *   susnet_observe         flatten_state base.py:234; FlatFeaturizer / GlobalFeaturizer
 *                          src/features/model_ready.py:219-370, src/features/component.py:83-482
 *   susnet_featurize       SequenceStateFeaturizer.fit(state_sequence[B,T,S]) on windows / replay batches
 *                          src/features/model_ready.py:41-57, 254-289, 338-354 (callers: src/train.py:345-347)
 *   susnet_scent           ImposterScentFeaturizer.extract_features   src/features/component.py:336-380
 *   susnet_dqn_train_step  DQNTeamTrainer.train_step on ReplayBuffer.sample's rows  src/train.py:50-149, src/replay_memory.py:75-94
 *   susnet_dqn_train_sweep the same for several learners at once: the sweeps over run_experiment(**config) of
 *                          notebooks/experiment_1v1.ipynb and notebooks/experiment_mlp.ipynb
 *   susnet_episode_stats   train()'s episode bookkeeping: G = reward + gamma * G, the teams' mean returns, episode lengths  src/train.py:385-450
 *   susnet_seed / _tick    np.random.seed(seed)            src/environment/base.py:126,267 (production stream)
 *   susnet_device_tick     (new) step counter in device memory: captured launches replay as a hipGraph
 *   susnet_bind_tape       (numpy's own MT19937 words: decisions equal the reference's for that seed)
 *   susnet_export_state    the state tuple step()/reset() return (base.py:317-324, 397-402)
 *   susnet_import_state    direct assignment to env.agent_positions etc. (what callers/tests do)
 *
 * Conventions
 *   - plain C types only; every device buffer is a caller-owned pointer (the Python host passes
 *     torch-ROCm tensor data_ptr()s); the library never allocates or frees device memory.
 *   - every call returns 0 on success or a negative SUSNET_E_* code; susnet_last_error() gives text.
 *   - all launches are asynchronous on the hipStream_t passed as `stream` (void*; NULL = default).
 *   - per-environment input errors (reference AssertionError / IndexError) are recorded in a device
 *     error word and reported by susnet_poll_errors(); an environment with a bad action is not stepped.
 *   - a handle is owned by one host thread; distinct handles are independent.
 */
#ifndef SUSNET_H
#define SUSNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUSNET_ABI_VERSION 8

#define SUSNET_MAX_AGENTS 16
#define SUSNET_MAX_JOBS 16
#define SUSNET_MAX_GRID 16
#define SUSNET_N_METRICS 13 /* SusMetrics, src/metrics.py:7-20, in declaration order */
#define SUSNET_N_LIFETIME 12

/* variant = reference class */
#define SUSNET_VARIANT_BASE 0
#define SUSNET_VARIANT_ITG 1
#define SUSNET_VARIANT_TAGGING 2

/* word source of all random decisions */
#define SUSNET_RNG_TAPE 1   /* caller-supplied raw 32-bit words consumed with numpy-legacy semantics:
                               given numpy's MT19937 output for seed s, results equal the reference's */
#define SUSNET_RNG_PHILOX 2 /* Philox4x32-10 keyed (seed, global env id): production stream */

/* error codes */
#define SUSNET_OK 0
#define SUSNET_E_INVALID (-1)  /* bad argument / config (reference ctor asserts, base.py:243-249) */
#define SUSNET_E_HIP (-2)      /* a HIP call failed */
#define SUSNET_E_STATE (-3)    /* state not bound */
#define SUSNET_E_ACTION_ASSERT (-4) /* some env got action >= action_space.n (base.py:360-362) */
#define SUSNET_E_ACTION_INDEX (-5)  /* some env got a role-invalid action index (base.py:379-382) */
#define SUSNET_E_TAPE (-6)     /* random tape exhausted */
#define SUSNET_E_ROW (-7)      /* susnet_featurize: a state row holds a coordinate outside the grid */

/* bits of the device error word */
#define SUSNET_ERRBIT_ASSERT 1u
#define SUSNET_ERRBIT_INDEX 2u
#define SUSNET_ERRBIT_TAPE 4u
#define SUSNET_ERRBIT_ROW 8u

/* dtypes of caller buffers */
#define SUSNET_U8 0
#define SUSNET_I32 1
#define SUSNET_I64 2
#define SUSNET_F32 3
#define SUSNET_F64 4

/* action / reward buffer layouts */
#define SUSNET_LAYOUT_AB 0 /* [A][B]  agent-major (SoA, what the kernels prefer) */
#define SUSNET_LAYOUT_BA 1 /* [B][A]  env-major (what reference callers index as actions[b]) */

/* observation modes (susnet_obs_spec.mode) */
#define SUSNET_OBS_NONE 0
#define SUSNET_OBS_RAW 1    /* flatten_state: [x0,y0,..., alive.., jobxy.., jobdone.. (, used, counts, timer_left)] */
#define SUSNET_OBS_FLAT 2   /* concatenation of flat components, FlatFeaturizer */
#define SUSNET_OBS_PLANES 3 /* GlobalFeaturizer: spatial [A+2][N][N] + non_spatial [A(+A)+J] */
#define SUSNET_OBS_PERSP 4  /* PerspectiveFeaturizer (model_ready.py:82-216): per agent i the planes with the agent channels in
                               the order i, 0, .., i-1, i+1, .., A-1 (then the two job channels): spatial [A][A+2][N][N];
                               non_spatial [A][A(+A)+J] = alive (and tag counts) in that same agent order, then job status */
/* The PERSP views under partial observability (PartiallyObservableFeaturizer, src/features/component.py:162-197 with ROOM_MASKS 8-17,
 * made total).  The room of cell (x, y) is (x <= w, y <= w), w = (N - 1) / 2: at N = 9 the reference's four quadrants, the wall row and
 * column with the top and the left rooms; a function of N alone, not of the wall map.  Every plane of agent i's view is multiplied by
 * the mask of the room that holds agent i's position in THAT state row (a dead agent keeps its stored position: its own channel is
 * blank, its mask is still its room's).  non_spatial (out2) is PERSP's, unmasked: the alive flags stay global.
 * out / out2 need only be aligned to their element type here (16 bytes gives vector stores; otherwise every element is stored singly).
 * Served by susnet_featurize and susnet_obs_size only: susnet_reset / susnet_step / susnet_rollout / susnet_observe and the policy
 * ticks refuse the two modes (SUSNET_E_INVALID) before any launch -- their kernels share one observation writer, which stays as it is. */
#define SUSNET_OBS_PERSP_ROOM 5      /* spatial [A][A+2][N][N]: the PERSP planes times the observer's room mask */
#define SUSNET_OBS_PERSP_ROOM_MASK 6 /* spatial [A][A+3][N][N]: the same, then the mask itself as the last channel
                                        (add_obs_mask_feature, the reference's default) */

/* flat components (src/features/component.py) */
#define SUSNET_F_ONEHOT_POS 0
#define SUSNET_F_COORD_POS 1
#define SUSNET_F_ALIVE_CREW 2
#define SUSNET_F_L1_CREW 3
#define SUSNET_F_CLOSEST_CREW 4
#define SUSNET_F_WALLS3X3 5
#define SUSNET_F_DIST_TO_IMP 6
#define SUSNET_F_ROOM_LOC 7

/* lifetime accumulator rows (per env, summed over finished episodes) */
#define SUSNET_L_EPISODES 0
#define SUSNET_L_CREW_WON 1
#define SUSNET_L_IMPOSTER_WON 2
#define SUSNET_L_TRUNCATED 3
#define SUSNET_L_KILLS 4
#define SUSNET_L_COMPLETED_JOBS 5
#define SUSNET_L_SABOTAGED_JOBS 6
#define SUSNET_L_IMP_VOTED_OUT 7
#define SUSNET_L_CREW_VOTED_OUT 8
#define SUSNET_L_EPISODE_STEPS 9
#define SUSNET_L_ENV_STEPS 10 /* every step the env took, finished episode or not (k_step: +1, a fused rollout: +n_ticks) */
#define SUSNET_L_RESERVED 11

typedef struct susnet_env susnet_env; /* opaque host-side handle */

/* Constructor arguments: the reference's ctor kwargs (base.py:103-120; pred_prey.py:26-38;
 * tagging.py:10-12) plus what a batched device env needs. */
typedef struct susnet_config {
    uint32_t struct_bytes; /* = sizeof(susnet_config) */
    uint32_t abi_version;  /* = SUSNET_ABI_VERSION */
    int32_t variant;
    int32_t batch;         /* environments on THIS device */
    int32_t n_imposters, n_crew, n_jobs;
    int32_t grid_n;        /* N; reference hard-codes 9 (base.py:195,206-207) */
    uint16_t grid_rows[SUSNET_MAX_GRID]; /* bit j of grid_rows[i] = grid[i][j], 1 = free (base.py:195-197) */
    double kill_reward, complete_job_reward, sabotage_reward, time_step_reward;
    double game_end_reward, dead_penalty, vote_reward;
    int32_t max_time_steps;
    int32_t is_action_order_random;
    int32_t shuffle_imposter_index;
    int32_t tag_reset_interval;
    int32_t auto_reset;    /* 1: an env that ends (done|truncated) is reset inside the same launch */
    int32_t rng_mode;      /* SUSNET_RNG_* */
    uint64_t seed;         /* Philox key */
    uint64_t env_id_base;  /* global id of local env 0 (sharding across GPUs keeps streams identical) */
    int32_t device;        /* HIP device ordinal the buffers live on */
    int32_t reserved;
} susnet_config;

/* Sizes the caller must allocate. All device buffers are raw bytes. */
typedef struct susnet_layout {
    uint64_t state_bytes;     /* the compact SoA state blob (see DESIGN.md "Data layout in HBM") */
    uint64_t state_align;     /* required alignment of the blob (256) */
    int32_t batch_padded;     /* SoA row stride in elements */
    int32_t n_agents;
    int32_t n_actions_imposter; /* len(agent_action_map[i]) for an imposter / a crew member */
    int32_t n_actions_crew;
    int32_t action_space_n;   /* Discrete(n) of the reference (8, or 8 + A with tagging) */
    int32_t obs_raw_size;     /* flattened_state_size (base.py:230-232) */
    int32_t envs_per_wave;    /* environments a wavefront of the fused rollout serves (64, 32 or 16, by batch size) */
    uint32_t test_overrides;  /* SUSNET_OVERRIDE_* bits: which test hooks were found in the environment at susnet_create */
} susnet_layout;

/* Test hooks.  Four environment variables change how a handle launches its kernels (never what it computes); they are read
 * ONCE, in susnet_create, recorded in susnet_layout.test_overrides, and named in susnet_last_error() messages of that handle:
 *   SUSNET_FORCE_GENERIC=1      every configuration runs the generic (LDS-table) kernels, none of the compiled-in ones
 *   SUSNET_EPW=16|32|64         environments per wave of the fused rollout
 *   SUSNET_TRAJ_MAX_BYTES=n     default of susnet_set_launch_limit()
 *   SUSNET_RING_TILE=0|8|16|32  susnet_ring_append: environments of a wave's (ticks x envs) tile; 0 (default) = 64 consecutive rows per wave */
#define SUSNET_OVERRIDE_FORCE_GENERIC 1u
#define SUSNET_OVERRIDE_EPW 2u
#define SUSNET_OVERRIDE_TRAJ_MAX_BYTES 4u
#define SUSNET_OVERRIDE_RING_TILE 8u

typedef struct susnet_obs_spec {
    int32_t mode;                 /* SUSNET_OBS_* */
    int32_t dtype;                /* SUSNET_F32 (reference layouts) or SUSNET_U8 (compact) */
    int32_t n_components;         /* FLAT only */
    int32_t components[16];       /* SUSNET_F_* in concatenation order */
    void *out;                    /* [B][obs_size]; PLANES: spatial [B][A+2][N][N]; PERSP, PERSP_ROOM: [B][A][A+2][N][N];
                                     PERSP_ROOM_MASK: [B][A][A+3][N][N] */
    void *out2;                   /* PLANES: non_spatial [B][A(+A)+J]; PERSP: [B][A][A(+A)+J]; else NULL */
} susnet_obs_spec;

/* The info counters of ONE finished episode: what the reference's `info` dict holds on the terminal step (EnvMetricHandler,
 * src/metrics.py:35-64) and metrics.step(info) appends to the run's per-episode lists (src/train.py:419-427).  16 bytes, 16-byte
 * aligned: the stepping lane writes it with one vector store where the episode ends, before the in-launch reset clears the counters.
 * Kills and votes are a byte each: an episode played from its reset kills at most n_crew <= 15 agents and votes out at most 16; only
 * imported states (susnet_import_state) can count further, and imp_killed_crew then saturates at 255.  TOTAL_STALEMATES has no field:
 * the reference never increments it. */
#define SUSNET_OUTCOME_CREW_WON 1u     /* bits of susnet_episode_info.outcome: SusMetrics.CREW_WON / IMPOSTER_WON */
#define SUSNET_OUTCOME_IMPOSTER_WON 2u
typedef struct susnet_episode_info {
    uint32_t time_steps;      /* TOTAL_TIME_STEPS: the steps of the episode */
    uint32_t completed_jobs;  /* COMPLETED_JOBS */
    uint32_t sabotaged_jobs;  /* SABOTAGED_JOBS */
    uint8_t imp_killed_crew;  /* IMP_KILLED_CREW */
    uint8_t imp_voted_out;    /* IMP_VOTED_OUT */
    uint8_t crew_voted_out;   /* CREW_VOTED_OUT */
    uint8_t outcome;          /* SUSNET_OUTCOME_* (0: truncated without a winner) */
} susnet_episode_info;

typedef struct susnet_step_io {
    const void *actions;  /* role-relative action indices (base.py:379-382) */
    int32_t actions_dtype;  /* SUSNET_U8 / I32 / I64 */
    int32_t actions_layout; /* SUSNET_LAYOUT_* */
    void *rewards;        /* out, one per agent */
    int32_t rewards_dtype;  /* SUSNET_F32 / F64 (reference: float64, base.py:369) */
    int32_t rewards_layout;
    uint8_t *done;        /* out [B]  (base.py:384-385) */
    uint8_t *truncated;   /* out [B]  (base.py:392-395) */
    const susnet_obs_spec *obs; /* optional fused observation of the post-step (post-auto-reset) state */
    /* replay feed of ONE tick (what susnet_ring_append needs besides actions / rewards / done / truncated / the raw uint8 observation
     * when the trajectory is collected tick by tick -- the trainer's loop, train.py:345-399 -- instead of by a fused rollout); both
     * optional: */
    uint8_t *term_obs;    /* out [B][obs_raw_size] u8, written ONLY where the episode ended at this step: its true terminal state
                           * (flatten_state order), before the auto-reset replaces it */
    uint16_t *roles;      /* out [B]: imposter bitmask (bit i = agent i) of the episode that acted at this step */
    susnet_episode_info *ep_info; /* out [B] or NULL, 16-byte aligned: written ONLY where the episode ended at this step (done | truncated),
                                   * next to term_obs: the episode's info counters, before the auto-reset clears them */
} susnet_step_io;

/* Fused random rollout: T lockstep ticks in one launch; per tick every env samples uniform role-valid
 * actions (sample_actions), steps, and auto-resets on done|truncated.  Every trajectory pointer is
 * optional (NULL = not stored).  PHILOX handles: any subset of outputs.  TAPE handles (numpy parity): the full trajectory
 * with the raw uint8 observation, as separate tensors or as packed records. */
typedef struct susnet_rollout_io {
    int32_t n_ticks;
    uint8_t *actions;   /* out [T][B][A] u8  (env-major: what reference callers index as actions[b]) */
    float *rewards;     /* out [T][B][A] f32 */
    uint8_t *done;      /* out [T][B] */
    uint8_t *truncated; /* out [T][B] */
    const susnet_obs_spec *obs; /* out pointer is [T][B][obs_size]; observation AFTER each tick */
    void *record;       /* alternative to ALL of the above (which must then be NULL): one packed record per env-step,
                         * [T][B][record_bytes] -- the same fields, laid out for one wide store per lane
                         * (susnet_record_layout); only for the compiled-in configurations */
    /* replay feed (susnet_ring_append); both optional, both need obs = RAW / U8 next to the full trajectory (term_obs also goes with
     * `record` on handles whose records are whole -- susnet_record_layout_t.planar == 0) */
    uint8_t *term_obs;  /* out [T][B][obs_raw_size] u8, written ONLY at (tick, env) where the episode ended: the true
                         * post-step state (the obs row of such a tick already holds the next episode's first state) */
    uint16_t *roles;    /* out [T][B]: imposter bitmask (bit i = agent i) of the episode that acted at the tick */
    int32_t record_format; /* which record `record` receives: SUSNET_RECORD_DEFAULT, or SUSNET_RECORD_COMPACT where the handle has one
                            * (susnet_record_layout_of) */
} susnet_rollout_io;
#define SUSNET_RECORD_DEFAULT 0
/* the 1v1 game on a grid without walls (BASELINE configs[1]): 16 bytes -- rewards f32[2] | raw observation u8[6] | ONE byte holding
 * actions and flags (susnet_record_layout_t.flags_packed) | 0 -- so that an env-step is one 16-byte store and a wave writes 1 KiB of
 * consecutive bytes per tick (+8 % env-steps/s over the 20-byte default, whose bytes stay as they are) */
#define SUSNET_RECORD_COMPACT 1

/* Device replay ring fed from a fused rollout: the reference's ReplayBuffer tensors (src/replay_memory.py:33-44) written by
 * ONE launch from the [T][B] trajectory of susnet_rollout, with ReplayBuffer.populate's semantics (replay_memory.py:96-143):
 * row n = tick * B + env (the order B sequential `add` calls per tick would produce) lands at ring position (idx + n) %
 * max_size; states[row] is the env's window of its last `trajectory_size` flattened states before the tick (after a reset:
 * the episode's first state repeated, replay_memory.py:108-113), next_states[row] the window rolled by one with the TRUE
 * post-step state appended (np.roll, replay_memory.py:120-127 -- also for a transition that ends its episode: term_obs),
 * dones[row] = done (not truncated), imposters[row] = ascending agent indices of the acting episode's imposters.  If the
 * launch holds more than max_size transitions only the last max_size are written.  `window` carries every env's window
 * across launches: in = before the first tick, out = before the tick that follows the last one. */
typedef struct susnet_ring_io {
    int32_t n_ticks;            /* T of the rollout */
    int32_t trajectory_size;    /* window length (ReplayBuffer.trajectory_size) */
    const uint8_t *actions;     /* [T][B][A] u8 */
    const float *rewards;       /* [T][B][A] */
    const uint8_t *done;        /* [T][B] */
    const uint8_t *truncated;   /* [T][B] */
    const uint8_t *obs;         /* [T][B][S] raw u8: state after each tick (after the in-launch reset, if any) */
    const uint8_t *term_obs;    /* [T][B][S] raw u8, read where done | truncated */
    const uint16_t *roles;      /* [T][B], or NULL: the imposters are agents [0, n_imposters) */
    uint8_t *window;            /* in/out [B][trajectory_size][S] u8 */
    int64_t max_size, idx;      /* ring capacity (rows), position of the next row */
    float *states;              /* [max_size][trajectory_size][S] */
    float *next_states;         /* [max_size][trajectory_size][S] */
    int64_t *ring_actions;      /* [max_size][A] */
    float *ring_rewards;        /* [max_size][A] */
    uint8_t *ring_dones;        /* [max_size][1] */
    int16_t *ring_imposters;    /* [max_size][n_imposters] */
    /* alternative to actions / rewards / done / truncated / obs (which must then be NULL): the [T][B] packed records a fused rollout
     * wrote (susnet_rollout_io.record, format record_format), read in place -- for handles that store whole records
     * (susnet_record_layout_t.planar == 0: the 1v1 kernels); term_obs as above */
    const uint8_t *record;
    int32_t record_format;
} susnet_ring_io;
int susnet_ring_append(susnet_env *env, const susnet_ring_io *io, void *stream);

/* Packed trajectory record of susnet_rollout_io.record: rewards f32[A], actions u8[A], done u8, truncated u8 and the raw
 * observation u8[obs_raw_size] (flatten_state order) of one env-step, zero-padded to a multiple of 4 bytes.  The ORDER of the
 * fields depends on the kernel that serves the handle (the multi-agent kernels store the observation right behind the actions
 * and done / truncated behind it, so that its words go out unshifted): read the byte offsets below, do not assume them.
 * record_bytes = 0 when the handle's configuration has no packed mode (not one of the compiled-in games). */
typedef struct susnet_record_layout_t {
    int32_t record_bytes;
    int32_t off_rewards, off_actions, off_done, off_truncated, off_obs;
    /* planar = 0: the record array is [T][B][record_bytes].
     * planar = 1 (the multi-agent kernels): the same record, cut into pieces of 16 bytes -- the last one(s) 8 and / or 4 bytes when
     * record_bytes is not a multiple of 16 -- and stored piece by piece, [T][piece][B][piece width]: every store instruction of a
     * wave then writes 1 KiB of consecutive bytes (40 partially written cache lines at a 40-byte record stride otherwise).  Byte o
     * of env b's record of tick t lives at
     *     t * B * record_bytes + B * P(o) + b * W(o) + (o - P(o)),
     * P(o) = the start of o's piece, W(o) its width: with full = record_bytes / 16 * 16, P(o) = o / 16 * 16, W = 16 for o < full;
     * then an 8-byte piece when record_bytes - full >= 8, then a 4-byte piece when record_bytes - full is 4 or 12. */
    int32_t planar;
    /* The raw observation (flatten_state order, obs_raw_size bytes) as the concatenation of n_obs_segments byte ranges of the record.
     * One segment (off_obs, obs_raw_size) for the fully compiled-in games; the multi-agent FAMILY kernels (any job count up to 8)
     * keep a record layout that does not depend on the job count -- eight job slots -- and report up to four segments: cells + alive,
     * job cells, job status, the tagging tail.  off_obs = the first segment's offset. */
    int32_t n_obs_segments;
    struct { int32_t off, len; } obs_segments[4];
    /* flags_packed = 1 (SUSNET_RECORD_COMPACT, two agents): off_actions = off_done = off_truncated = ONE byte
     * a0 | a1 << 3 | done << 6 | truncated << 7 (role-relative action indices below 8). */
    int32_t flags_packed;
} susnet_record_layout_t;
int susnet_record_layout(const susnet_env *env, susnet_record_layout_t *out);        /* the default record */
int susnet_record_layout_of(const susnet_env *env, int32_t record_format, susnet_record_layout_t *out); /* record_bytes = 0: the handle has no such record */

/* The trajectory modes of susnet_rollout address every output array with 32-bit offsets: one launch covers at most as many ticks
 * as keep each array below `bytes` (default and maximum 2^31 - 1); longer requests run as consecutive launches.  bytes = 0
 * restores the default.  (No reference counterpart: launch plumbing.) */
int susnet_set_launch_limit(susnet_env *env, uint64_t bytes);

/* Reference-layout views of the state (export / import). NULL pointers are skipped. */
typedef struct susnet_state_view {
    int32_t *agent_positions; /* [B][A][2] (x, y)            base.py:291 */
    uint8_t *alive_agents;    /* [B][A]                      base.py:301 */
    uint8_t *imposter_mask;   /* [B][A]                      base.py:280-281 */
    int32_t *job_positions;   /* [B][J][2]                   base.py:299 */
    uint8_t *completed_jobs;  /* [B][J]                      base.py:302 */
    uint8_t *used_tag_actions;/* [B][A]                      tagging.py:30 */
    int32_t *tag_counts;      /* [B][A]                      tagging.py:29 */
    int32_t *tag_reset_timer; /* [B]                         tagging.py:31 */
    int32_t *t;               /* [B]                         base.py:315 */
    int64_t *metrics;         /* [B][13] info counters       metrics.py:35-64 */
    uint64_t *rng_cursor;     /* [B] words consumed so far (PHILOX: the event stream = the kill draws; TAPE: every draw) */
    uint32_t *lifetime;       /* [SUSNET_N_LIFETIME][B] per-env sums over finished episodes */
    uint32_t *episode_index;  /* [B] resets drawn so far = the index of the env's next reset in the RESET stream (PHILOX handles:
                                 a reset's draws are a function of (seed, global env id, this index) alone) */
} susnet_state_view;

int susnet_abi_version(void);
const char *susnet_last_error(void);

int susnet_create(const susnet_config *cfg, susnet_env **out);
void susnet_destroy(susnet_env *env);
int susnet_get_layout(const susnet_env *env, susnet_layout *out);

/* Bind the caller-allocated state blob (zero-filled by the callee, asynchronously, on `stream`). */
int susnet_bind_state(susnet_env *env, void *state_blob, uint64_t bytes, void *stream);
/* TAPE mode: per-env raw 32-bit words, tape[b][0..words_per_env); cursors restart at 0. */
int susnet_bind_tape(susnet_env *env, const uint32_t *tape, int64_t words_per_env);
/* PHILOX mode: reseed / reposition every env's stream (also rewinds the handle's tick counter to 0). */
int susnet_seed(susnet_env *env, uint64_t seed, uint64_t cursor, void *stream);
/* PHILOX mode draws agent actions from a second stream indexed by the number of steps the handle has taken
 * ("tick"; advanced by susnet_step / susnet_rollout, NOT by susnet_sample_actions -- sampling twice before a
 * step returns the same actions).  Set and/or read it (either pointer may be NULL).  With the counter in device memory
 * (susnet_device_tick) both are ordered on `stream`; reading synchronises `stream`. */
int susnet_tick(susnet_env *env, const uint64_t *set, uint64_t *get, void *stream);

int susnet_reset(susnet_env *env, const uint8_t *mask /* [B] or NULL = all */, const susnet_obs_spec *obs,
                 void *stream);
int susnet_sample_actions(susnet_env *env, void *actions_out, int32_t dtype, int32_t layout, void *stream);

/* Greedy policy actions of one tick -- the acting step of the reference's policy loops (run_game, src/visualize.py:547-562:
 * every agent takes the argmax of ITS TEAM's Q-network; train.py:355-381 with epsilon = 0):
 *   actions[b][i] = argmax_k q_imposter[b][k]   if agent i is an imposter of environment b
 *                 = argmax_k q_crew[b][k]       otherwise
 * q_imposter / q_crew: float32 [B][n_actions_imposter] / [B][n_actions_crew], one row per environment (all agents of an
 * environment share the flat observation, FlatFeaturizer model_ready.py:356-367); ties go to the lowest index, like
 * torch.argmax / np.argmax.  q_crew = NULL: the crew draws uniformly random role-valid indices from the production action
 * stream -- exactly what susnet_sample_actions would return for them (PHILOX handles only).  One launch instead of the
 * role export + argmax + sample + dtype copy + where of the eager loop; actions_out as for susnet_sample_actions. */
typedef struct susnet_policy_opts {
    float epsilon;     /* epsilon-greedy, train.py:355-381: with this probability an agent takes its uniformly random role-valid draw (what
                        * susnet_sample_actions returns for it) instead of the argmax; the decision is word tick * A + i of a third
                        * stream of the handle's Philox key (PHILOX handles only); 0 = greedy */
    int32_t mask_dead; /* != 0: dead agents get index 0 (train.py sets only the living agents' actions); 0: they act like everybody
                        * else (run_game, visualize.py:547-560) -- the step ignores a dead agent's action either way */
    /* ABI 6 -- the CREW's Q-network inside the one-kernel tick (susnet_qnet_policy_step / susnet_qnet_policy_rollout only; the other
     * calls take the crew's Q rows as an argument and refuse these fields): run_game drives both teams by their networks
     * (visualize.py:547-562), train_crew exists (notebooks/experiment.ipynb cell 5).  crew_packed: a susnet_qnet_pack image for the SAME
     * components as the imposters' network (device, 16-byte aligned), crew_dims / crew_n_dims its layer widths (last = the crew's action
     * count), crew_q_out: [B][n] float32 (rollout: [T][B][n]) or NULL.  NULL crew_packed = a uniformly random crew.  With both networks and
     * epsilon = 0 nothing is drawn from the action stream, so numpy-tape (TAPE) handles are served as well. */
    const float *crew_packed;
    const int32_t *crew_dims;
    int32_t crew_n_dims, pad_;
    float *crew_q_out;
} susnet_policy_opts;
int susnet_policy_actions(susnet_env *env, const float *q_imposter, const float *q_crew, const susnet_policy_opts *opts /* or NULL */,
                          void *actions_out, int32_t dtype, int32_t layout, void *stream);

/* susnet_policy_actions with one Q row per AGENT -- the acting step of train() for a network that reads each agent's own view
 * (src/train.py:351-381 with a SpatialDQN: the Perspective featurizer gives every agent its view, the Global one its one-hot):
 *   actions[b][i] = argmax_k q_imposter[b][i][k]   if agent i is an imposter of environment b
 *                 = argmax_k q_crew[b][i][k]       otherwise
 * q_imposter / q_crew: float32 [B][A][n_actions_imposter] / [B][A][n_actions_crew], contiguous -- the [B * A][n] rows
 * susnet_spatial_forward writes with agents = A; the first maximum wins.  Everything else is susnet_policy_actions': the roles and alive
 * words, the action stream for the crew's draws and the sampled index, the exploration stream for u <= epsilon (draws for every agent),
 * mask_dead, q_crew = NULL = a random crew (PHILOX handles only), no draw at all with both networks and epsilon = 0 (TAPE handles are
 * served there).  With every agent's row equal to its environment's the two calls return the same bytes.  No limit on the number of
 * actions (rows are n_actions_* of susnet_get_layout long).  SUSNET_E_INVALID, naming the field, before any launch: NULL q_imposter /
 * actions_out, a dtype / layout outside the enums, a crew network in opts, q_crew = NULL or epsilon > 0 on a handle that is not PHILOX. */
int susnet_agent_policy_actions(susnet_env *env, const float *q_imposter, const float *q_crew, const susnet_policy_opts *opts /* or NULL */,
                                void *actions_out, int32_t dtype, int32_t layout, void *stream);

/* The policy loop's Q-network -- the reference's MLP (src/models/dqn.py:72-108: make_mlp 322-329, Linear + nn.PReLU() with ONE
 * slope per layer, no activation after the last Linear) on the FlatFeaturizer observation of the handle's CURRENT environments
 * (model_ready.py:356-367) -- as one kernel: MLP.forward(spatial, env.obs) without the observation or any activation ever
 * being written to memory (float32 throughout; layers 2.. on the f32-input matrix instructions, whose result is a k-ordered fmaf
 * chain, so values agree with torch's to float32 summation-order differences).  Served: five Linear layers
 * dims = [F, <=256, <=128, <=64, <=32, <=32] (the reference's [F, 256, 128, 64, 16, n_actions], notebooks/experiment_1v1.ipynb cell 1) on
 * the compiled-in feature layouts: components {ONEHOT_POS} (F = 36: experiments no_wall / one_hot_wall of notebooks/experiment_1v1.ipynb)
 * or {COORD_POS} (F = 4, CoordinateAgentPositionsFeaturizer, component.py:384-403: no_wall_coord_features / wall_coord_features) on the
 * 2-agent 9x9 game, either map, and {ONEHOT_POS, ALIVE_CREW, CLOSEST_CREW} on the 3-agent 14x14 game (F = 88).
 *   susnet_qnet_packed_floats  size of the packed weight image (floats), or SUSNET_E_INVALID when the handle / components / dims are
 *                              not served (callers then run the network themselves and hand Q rows to susnet_policy_actions);
 *   susnet_qnet_pack           HOST: torch-layout weights[l] ([dims[l+1]][dims[l]] row-major), biases[l] ([dims[l+1]]), slopes
 *                              ([n_dims - 2], the PReLU weights) -> packed (host buffer of that size; the caller copies it to the device:
 *                              the library never allocates device memory);
 *   susnet_qnet_forward        q_out [B][dims[n_dims-1]] float32 (device) from the packed image (device, 16-byte aligned). */
int64_t susnet_qnet_packed_floats(const susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims,
                                  int32_t n_dims);
int susnet_qnet_pack(const susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims, int32_t n_dims,
                     const float *const *weights, const float *const *biases, const float *slopes, float *packed);
int susnet_qnet_forward(susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims, int32_t n_dims,
                        const float *packed, float *q_out, void *stream);

/* The same network -- the reference's MLP.forward (src/models/dqn.py:72-108; make_mlp 322-329: Linear + nn.PReLU() with ONE slope per
 * layer, no activation after the last Linear) -- of ANY served layer stack on CALLER-SUPPLIED feature rows: every game, component set and
 * layer stack the compiled-in family above does not know.  rows: [n][F] float32 contiguous -- env.obs of a FLAT observation, the output of
 * susnet_observe / susnet_featurize in FLAT mode, or anything else; q_out: [n][n_out].
 *   Weights are read where torch keeps them: weight[l] is the module's parameter tensor ([dims[l+1]][dims[l]] row-major; only 4-byte
 * alignment is assumed), bias[l] its bias, slope[l] the one-element PReLU weight behind layer l.  There is no packed image and no host step:
 * after an in-place optimizer step (torch's, or susnet_dqn_train_step on a flat parameter buffer) the next launch reads the new values.
 *   Served: 1 .. 7 Linear layers (n_dims 2 .. 8), F = dims[0] in 1 .. SUSNET_MLP_MAX_F (every flat layout of a 16-agent 16x16 game is
 * below it), hidden widths 1 .. 256, n_out = dims[n_dims-1] in 1 .. 32, n >= 1; rows / q_out / the parameter pointers non-NULL and 4-byte
 * aligned.  Anything else: SUSNET_E_INVALID, with a message that names the field, before anything is launched.
 *   Arithmetic: float32 throughout on the f32-input matrix instruction (v_mfma_f32_32x32x2_f32); as in susnet_qnet_forward every output is
 * ONE chain over k in ascending order whose accumulator starts as the bias, so values agree with torch's to float32 summation-order
 * differences.  No activation goes through global memory; the weights are streamed from global memory / L2 by every workgroup.
 *   One launch of at most SUSNET_MLP_MAX_GRID workgroups, each walking tiles of SUSNET_MLP_ROW_TILE rows.  The handle supplies the stream
 * and error conventions only: no environment state is read, and the handle need not have its state bound. */
#define SUSNET_MLP_MAX_F 1024
#define SUSNET_MLP_ROW_TILE 64
#define SUSNET_MLP_MAX_GRID 512
typedef struct susnet_mlp_io {
    int32_t n_dims;            /* 2 .. 8: 1 .. 7 Linear layers */
    int32_t dims[8];           /* [F, h1, .., n_out] */
    const float *weight[7];    /* device, torch layout [dims[l+1]][dims[l]] row-major, 4-byte aligned only */
    const float *bias[7];      /* device [dims[l+1]] */
    const float *slope[6];     /* device [1] each: the PReLU weight behind layer l (n_dims - 2 of them) */
    const float *rows;         /* device [n][F] float32, contiguous (env.obs / susnet_observe / susnet_featurize FLAT output) */
    int64_t n;
    float *q_out;              /* device [n][n_out] float32 */
} susnet_mlp_io;
int susnet_mlp_forward(susnet_env *env, const susnet_mlp_io *io, void *stream);

/* The reference's SpatialDQN.forward (src/models/dqn.py:205-301) in EVAL mode, float32, on the featurizers' (spatial, non_spatial) tensors
 * where they lie.  Row r of n is (env r / agents, agent r % agents); its window holds T steps.  Per row and step t:
 *     image [C][N][N] = spatial + env * spatial_stride[0] + agent * spatial_stride[1] + t * spatial_stride[2]      (floats)
 *     -> n_conv x { Conv2d(k x k, stride, padding, dilation) + ReLU }   (CNNModel, dqn.py:141-181; the reference's repeated last layer is
 *        simply one more entry of the lists here)
 *     -> flattened in torch's [C_out][H][W] order, that step's Fn non-spatial features (non_spatial + the same three kinds of stride)
 *        appended (the view and torch.cat of dqn.py:292-294): one row of rnn_in [n][T][R], R = conv_out[n_conv-1] * H_out^2 + Fn
 *     -> nn.RNN(tanh, batch_first, num_layers = rnn_layers) over the T rows from h = 0 (RNNModel, dqn.py:184-202, 296)
 *     -> the PReLU head -- make_mlp, as susnet_mlp_forward: Linear + nn.PReLU() with ONE slope per layer, none after the last Linear -- on
 *        the last layer's hidden state at t = T - 1 (dqn.py:298-299): q_out [n][dims[n_dims-1]].
 *   The PERSPECTIVE featurizer's buffers are served in place (spatial [B][T][A][C][N][N]: strides T*A*C*N*N, C*N*N, A*C*N*N), and so are the
 * GLOBAL featurizer's shared planes ([B][T][C][N][N] with an agent stride of 0: the image's convolution is then recomputed per agent).
 *   EVAL-mode semantics: there is no dropout in these kernels (nn.RNN's dropout between layers acts in training mode only);
 * susnet_spatial_forward_dropout, declared with the dropout entry points below, is the training-mode form of this call.
 *   Parameters are read where torch keeps them, as susnet_mlp_forward reads them: conv_weight[l] [conv_out[l]][C_in][k][k], w_ih[l]
 * [rnn_hidden][R or rnn_hidden], w_hh[l] [rnn_hidden][rnn_hidden], the head's weight[l] [dims[l+1]][dims[l]], all row-major and only 4-byte
 * aligned; no packed image, no host step: after an in-place optimizer step the next launch reads the new values.
 *   Summation orders (float32 throughout): a convolution output is ONE fmaf chain that starts as the bias and runs over (c_in, ky, kx) in
 * ascending order, padding taps being zeros; a recurrent unit's accumulator starts as b_ih + b_hh, then k ascends over W_ih (x_t, or the
 * layer below's h at t), then over W_hh (the layer's own h at t - 1; nothing is added at t = 0), and tanh is applied to the result; the
 * head's outputs are chains over k ascending that start as the bias.  tanh(x) is copysign(-e / (e + 2), x) with e = expm1f(-2 |x|): exactly
 * 0 at 0 and exactly +-1 for |x| >= 16.  Values agree with torch's to float32 summation-order and tanh rounding differences.
 *   Served: T in 1 .. 8, N in 1 .. 16, C in 1 .. 32; n_conv in 1 .. 4, conv_out[l] in 1 .. 32, k in {1, 3, 5}, conv_stride[l] in 1 .. 4,
 * conv_padding[l] in 0 .. 8, conv_dilation[l] in 1 .. 4, every layer's output size (size + 2 padding - dilation (k - 1) - 1) / stride + 1 at
 * least 1; Fn >= 0; R <= SUSNET_SPATIAL_MAX_R; rnn_layers in 1 .. 4, rnn_hidden in 1 .. 256; the head n_dims in 2 .. 8 with dims[0] ==
 * rnn_hidden, hidden widths 1 .. 256 and at most 32 outputs; n >= 1, agents >= 1, strides >= 0; every pointer non-NULL and 4-byte aligned
 * (with Fn == 0 nothing is read through non_spatial: NULL is accepted there -- a [B][T][0] tensor has no storage -- a pointer that is given
 * must still be 4-byte aligned, and non_spatial_stride is not looked at);
 * the LDS of a call within a workgroup's 160 KiB: one image's two activation buffers for the convolutions, and (rnn_layers + 1) x 64 rows x
 * max(rnn_hidden, the head's hidden widths) floats for the recurrence (so rnn_hidden 256 is served with one layer, 128 with up to four).
 * Anything else: SUSNET_E_INVALID, with a message that names the field, before anything is launched.
 *   Two launches: the convolutions on the vector ALU (at most SUSNET_SPATIAL_CONV_MAX_GRID workgroups walking groups of up to
 * SUSNET_SPATIAL_CONV_GROUP images), the recurrence and the head on v_mfma_f32_32x32x2_f32 (the tiles and grid of susnet_mlp_forward).  rnn_in
 * is caller-supplied workspace, written whole.  The handle supplies the stream and error conventions only. */
#define SUSNET_SPATIAL_MAX_T 8
#define SUSNET_SPATIAL_MAX_N 16
#define SUSNET_SPATIAL_MAX_C 32
#define SUSNET_SPATIAL_MAX_CONV 4
#define SUSNET_SPATIAL_MAX_R 4096
#define SUSNET_SPATIAL_MAX_RNN_LAYERS 4
#define SUSNET_SPATIAL_CONV_GROUP 16
#define SUSNET_SPATIAL_CONV_MAX_GRID 1024
typedef struct susnet_spatial_io {
    int32_t T, N, C;                 /* window steps, image size, input channels */
    int32_t n_conv, k;               /* 1 .. 4 convolutions of one square kernel size k in {1, 3, 5} */
    int32_t conv_out[4], conv_stride[4], conv_padding[4], conv_dilation[4];
    const float *conv_weight[4];     /* device [conv_out[l]][C_in][k][k] */
    const float *conv_bias[4];       /* device [conv_out[l]] */
    int32_t Fn;                      /* non-spatial features per step */
    int32_t rnn_layers, rnn_hidden;
    const float *w_ih[4], *w_hh[4], *b_ih[4], *b_hh[4]; /* nn.RNN's weight_ih_l{l} .. bias_hh_l{l} */
    int32_t n_dims;                  /* the head, as susnet_mlp_io: 2 .. 8 */
    int32_t dims[8];                 /* [rnn_hidden, h1, .., n_actions] */
    const float *weight[7];
    const float *bias[7];
    const float *slope[6];
    const float *spatial;            /* device float32 */
    int64_t spatial_stride[3];       /* floats: per env, per agent, per timestep; an image [C][N][N] is contiguous */
    const float *non_spatial;        /* device float32 */
    int64_t non_spatial_stride[3];   /* floats: per env, per agent, per timestep; a step's Fn features are contiguous */
    int32_t agents;                  /* row r is env r / agents, agent r % agents */
    int64_t n;                       /* rows */
    float *rnn_in;                   /* device workspace [n][T][R] float32 */
    float *q_out;                    /* device [n][dims[n_dims-1]] float32 */
} susnet_spatial_io;
int susnet_spatial_forward(susnet_env *env, const susnet_spatial_io *io, void *stream);

/* The trainer's state window (src/train.py:318-322, 388-389, 441-445) as FEATURE rows on the device, one tick on.  The reference keeps the
 * last T flattened states per env, featurizes all T every tick (FlatFeaturizer.fit, src/features/model_ready.py:325-354) and MLP.forward
 * flattens the [B, T, F] features into one T * F wide input, oldest state first (src/models/dqn.py:86-90).  Here the window is kept
 * featurized: a row of T segments of F floats -- an input row of susnet_mlp_forward / susnet_mlp_train_step with dims[0] = T * F -- and per
 * tick only the new state's row (fresh) is produced.  Per row b, with ended = (done && done[b]) || (truncated && truncated[b]):
 *     ended      dst[b] = fresh[b] repeated T times    (train.py:441-445: the window is refilled with the fresh first state; 318-322 at start)
 *     otherwise  dst[b] = src[b][F:] ++ fresh[b]       (train.py:388-389: np.roll(-1), the last slot is the new state)
 *   OUT OF PLACE by design: dst must not overlap src (nor fresh); callers ping-pong two buffers.  Values move as 32-bit patterns: NaN payloads
 * and -0.0 survive.  done / truncated are read in place, e.g. a slot of the replay feed the stepping kernel has just written.
 *   Served: T in 1 .. 8, F >= 1, T * F <= SUSNET_MLP_MAX_F, n >= 1; fresh / src / dst non-NULL and 4-byte aligned (rows of arbitrary F are
 * only 4-byte aligned: every access is one dword), the byte ranges of src and dst disjoint.  Anything else: SUSNET_E_INVALID, with a
 * message that names the field, before anything is launched.
 *   One launch (grid-stride over chunks of rows), no LDS, no atomics.  The handle supplies the stream and error conventions only: no
 * environment state is read, and the handle need not have its state bound. */
typedef struct susnet_window_io {
    const float *fresh;       /* device [n][F]: FlatFeaturizer row of the state AFTER the tick (after the auto-reset where the episode ended) */
    const uint8_t *done;      /* device [n] or NULL */
    const uint8_t *truncated; /* device [n] or NULL */
    const float *src;         /* device [n][T*F]: the window before the tick, oldest state first */
    float *dst;               /* device [n][T*F]: the window after it; must not overlap src */
    int32_t T, F;
    int64_t n;
} susnet_window_io;
int susnet_window_push(susnet_env *env, const susnet_window_io *io, void *stream);

/* The acting loop's RAW state window (src/train.py:388-389, 441-445), one tick on, IN PLACE: window is device uint8 [n][T][S], oldest
 * state first -- the carried window susnet_ring_append keeps (susnet_ring_io.window).  obs / done / truncated: ONE slot of the replay feed
 * as the stepping kernel wrote it ([n][S] uint8: the state after the tick, after the auto-reset where the episode ended; [n] flags), read
 * in place.  Per environment b:
 *     done[b] | truncated[b]   window[b] = obs[b] repeated T times      (train.py:441-445)
 *     otherwise                window[b] = window[b][1:] ++ obs[b]      (train.py:388-389: np.roll(-1), the last slot is the new state)
 * This is susnet_ring_append's own window kernel launched for one tick, so an acting window moved by this call and the ring's carried
 * window follow the same code.  Served: T in 1 .. 8, S = obs_raw_size of the handle, n = its batch, all four pointers non-NULL; anything
 * else is SUSNET_E_INVALID naming the field, before the launch.  No environment state is read: the handle need not have its state bound. */
int susnet_state_window_push(susnet_env *env, uint8_t *window, int32_t T, int32_t S, int64_t n, const uint8_t *obs, const uint8_t *done,
                             const uint8_t *truncated, void *stream);

int susnet_step(susnet_env *env, const susnet_step_io *io, void *stream);
/* susnet_policy_actions and susnet_step in ONE launch -- a tick of the acting loop (visualize.py:547-582: argmax per team, env.step):
 * the stepping lane takes the teams' greedy actions from the Q rows itself (q_imposter / q_crew as for susnet_policy_actions; at most
 * 16 actions per team) and steps with them; io->actions is an OUTPUT here (the actions taken, same dtypes / layouts; NULL: not kept),
 * every other field of io as for susnet_step. */
int susnet_policy_step(susnet_env *env, const float *q_imposter, const float *q_crew, const susnet_policy_opts *opts /* or NULL */,
                       const susnet_step_io *io, void *stream);
/* susnet_qnet_forward and susnet_policy_step (imposters by the network; the crew random, or by ITS network: opts->crew_packed) as ONE
 * kernel -- a whole tick of the acting loop in one launch: the wave that computed its 64 environments' Q rows takes their argmax in
 * registers and steps them (with a crew network the workgroup swaps the LDS image between the two passes).  Arguments as for
 * the two calls; q_out may be NULL (Q rows not kept).  Served: the two compiled-in games on the three feature layouts the network kernel
 * knows (2-agent 9x9 ImposterTrainingGround, either map, with {ONEHOT_POS} or {COORD_POS}; 1v2 14x14 FourRoomEnv with 4 jobs with
 * {ONEHOT_POS, ALIVE_CREW, CLOSEST_CREW}).  PHILOX handles with a random crew or the crew's network and any epsilon; TAPE handles with
 * both networks and epsilon = 0 (nothing is drawn then).  Otherwise SUSNET_E_INVALID and the caller uses the two calls. */
int susnet_qnet_policy_step(susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims, int32_t n_dims,
                            const float *packed, float *q_out, const susnet_policy_opts *opts /* or NULL */, const susnet_step_io *io, void *stream);

/* The policy tick (susnet_qnet_policy_step) repeated n_ticks times inside ONE launch: the acting loop of the trainer over a block of
 * ticks with fixed weights (train.py:345-399 between two optimizer steps) -- the network image is loaded once, a launch is paid once,
 * and what replay_buffer.add needs of every tick lands in slot t of [T][B] arrays, ready for susnet_ring_append.  Every pointer is
 * optional.  Served where susnet_qnet_policy_step is (the two compiled-in games on their three feature layouts; PHILOX handles with a random
 * crew or the crew's network through opts->crew_*, TAPE handles with both networks at epsilon = 0); the handle must auto-reset.  Advances
 * the handle by n_ticks steps. */
typedef struct susnet_feed_io {
    uint8_t *actions;    /* out [T][B][A] u8: the actions taken */
    float *rewards;      /* out [T][B][A] f32 */
    uint8_t *done;       /* out [T][B] */
    uint8_t *truncated;  /* out [T][B] */
    uint8_t *obs;        /* out [T][B][obs_raw_size] u8: the state after each tick (after the auto-reset where the episode ended); 16-byte aligned
                          * slots (n_ticks > 1: B * obs_raw_size a multiple of 16, else SUSNET_E_INVALID) */
    uint8_t *term_obs;   /* out [T][B][obs_raw_size] u8, written only where an episode ended: its terminal state */
    uint16_t *roles;     /* out [T][B]: imposter bitmask of the episode that acted */
    float *q;            /* out [T][B][n_actions_imposter] f32: the imposters' Q rows, or NULL */
    susnet_episode_info *ep_info; /* out [T][B] or NULL, 16-byte aligned: written only where an episode ended: its info counters */
} susnet_feed_io;
int susnet_qnet_policy_rollout(susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims, int32_t n_dims,
                               const float *packed, const susnet_policy_opts *opts, const susnet_feed_io *feed, int32_t n_ticks, void *stream);

int susnet_rollout(susnet_env *env, const susnet_rollout_io *io, void *stream);
int susnet_observe(susnet_env *env, const susnet_obs_spec *obs, void *stream);
int susnet_obs_size(const susnet_env *env, const susnet_obs_spec *obs, int32_t *size_out, int32_t *size2_out);

/* Observation of n_rows FLATTENED states instead of the handle's own environments: what the reference's
 * sequence featurizers do with a state window or a replay batch -- SequenceStateFeaturizer.fit(state_sequence
 * [B, T, S]) un-flattens every state and featurises it (src/features/model_ready.py:41-57; FlatFeaturizer.fit
 * 338-354, GlobalFeaturizer.fit 254-289; the trainer calls it on windows train.py:345-347 and on replay batches).
 * rows: device pointer, [n_rows][S] contiguous, S = susnet_layout.obs_raw_size (flatten_state order, base.py:234:
 * x0,y0,.. alive.. jobxy.. jobdone.. (, used, counts, timer_left)), rows_dtype one of SUSNET_U8 / I32 / I64 / F32 /
 * F64 (integer-valued).  obs->out (/out2) receive [n_rows][obs_size] in the layouts of susnet_observe; obs->mode
 * FLAT, PLANES, PERSP, PERSP_ROOM or PERSP_ROOM_MASK.  A row with a coordinate outside the grid is written as all zeros and reported by
 * susnet_poll_errors (SUSNET_E_ROW).  The handle supplies the configuration (A, J, N, wall map) only; its
 * environments are not touched. */
int susnet_featurize(susnet_env *env, const void *rows, int32_t rows_dtype, int64_t n_rows, const susnet_obs_spec *obs,
                     void *stream);

/* ImposterScentFeaturizer (src/features/component.py:336-380; the one real-valued feature of the reference) of n_rows
 * FLATTENED states (layout and dtypes as susnet_featurize): out [n_rows][4] float32, 16-byte aligned. */
int susnet_scent(susnet_env *env, const void *rows, int32_t rows_dtype, int64_t n_rows, float *out, void *stream);

int susnet_export_state(susnet_env *env, const susnet_state_view *view, void *stream);
int susnet_import_state(susnet_env *env, const susnet_state_view *view, void *stream);

/* Sum the per-env lifetime accumulators into out[SUSNET_N_LIFETIME] (device int64 buffer): the vector
 * the multi-GPU host all-gathers.  One small launch. */
int susnet_reduce_lifetime(susnet_env *env, int64_t *out_device, void *stream);

/* Graph-replayable launches.  By default the step counter that indexes the production action stream (susnet_tick)
 * travels as a kernel argument, so a captured launch would replay with a stale value.  enable = 1 moves the counter
 * into device memory (inside the bound state blob), ONE COPY PER ENVIRONMENT: sample_actions / step / rollout read the
 * env's own copy and step / rollout advance it in the same kernel (the lane that owns the env; no extra launch, no word
 * one workgroup writes while another reads), so a hipGraph captured from these calls (e.g. {susnet_sample_actions;
 * susnet_step}) can be replayed any number of times.  enable = 0 reads it back (synchronises `stream`).  susnet_tick()
 * keeps working in both modes. */
int susnet_device_tick(susnet_env *env, int32_t enable, void *stream);

/* The learner's train step -- DQNTeamTrainer.train_step (src/train.py:50-149) on a replay batch drawn by index from the device ring
 * (ReplayBuffer.sample, src/replay_memory.py:75-94; the ring tensors of susnet_ring_io are read in place, nothing is gathered):
 * for agent i = 0 .. A-1, first the imposter team (rows with imposters[row][0] == i, train.py:83-84), then the crew team (the other
 * rows): Q = online(features(states))[rows, actions[rows][i]], y = rewards[rows][i] + gamma * max_a target(features(next_states))
 * (y = rewards on done rows, train.py:121-134; truncation ignored as there), loss = mean MSE (train.py:136), backward -- the
 * gradients ACCUMULATE over the agents, the reference zeroes them once per call (train.py:64-67) -- and one torch.optim.Adam step
 * (train.py:24-38: betas, eps, no weight decay; torch's single-tensor update order).  A team without rows in the batch takes no step
 * and its step count does not advance (train.py:101).  Everything is decided on the device: no host synchronisation, at most two
 * launches per (agent, team) update, one launch per call to split the batch and one per team to rewrite its packed image, so a
 * whole call can be captured as a hipGraph.  Sums of partials run in a fixed order: results are bitwise reproducible.
 * Served: what susnet_qnet_forward serves (the compiled-in feature layouts, dims [F, <=256, <=128, <=64, <=32, <=32]) with
 * trajectory_size == 1 and one imposter (the reference's own train_step fails on two: `(batch.imposters == agent_idx).view(-1)`,
 * train.py:83, has n_imposters * N entries); anything else returns SUSNET_E_INVALID and the caller runs the step in torch.
 * Input validity is the caller's: the kernels do not stop on bad data but keep every access in bounds -- an index outside
 * 0 .. max_size-1 is clamped into it, an action outside 0 .. n_actions-1 likewise, and a state row with a coordinate off the grid
 * featurizes as all zeros (where the reference would raise).  DeviceDQNTeamTrainer draws the indices itself, and the ring is written
 * by susnet_ring_append, whose rows are valid by construction. */
typedef struct susnet_dqn_team {
    int32_t enabled;          /* != 0: the team has an optimizer (OptimizerType.build returns None for a random model, train.py:33-34) */
    int32_t n_dims;           /* 6 */
    int32_t dims[8];          /* [F, h1, h2, h3, h4, n_actions] (MLP layer_dims, dqn.py:72-82) */
    double lr, beta1, beta2, eps; /* torch.optim.Adam(params, lr=learning_rate) (train.py:35-37): betas (0.9, 0.999), eps 1e-8 */
    float *params;            /* device, torch parameter order of MLP.parameters() (model.0.weight [h1][F], model.0.bias, model.1.weight (the
                               * PReLU slope), model.2.weight, ...), contiguous; updated in place */
    const float *target_params; /* the target network (train.py:341-343), same layout */
    float *exp_avg, *exp_avg_sq;  /* Adam state (torch's state['exp_avg'], state['exp_avg_sq']), same layout */
    float *step;              /* [1] float32: Adam's state['step'], advanced on the device */
    float *packed;            /* susnet_qnet_pack image of `params` to rewrite after the call (bitwise what the host packer makes), or NULL */
} susnet_dqn_team;
typedef struct susnet_dqn_io {
    int32_t n_components;     /* the FlatFeaturizer components the networks read (model_ready.py:309-367) */
    int32_t components[16];
    int32_t trajectory_size;  /* ring window T (replay_memory.py:33-44); 1 is served */
    const float *states;      /* ring [max_size][T][S] float32 (replay_memory.py:33-44) */
    const float *next_states; /* ring [max_size][T][S] float32 */
    const int64_t *actions;   /* ring [max_size][A] int64 */
    const float *rewards;     /* ring [max_size][A] float32 */
    const uint8_t *dones;     /* ring [max_size][1] bool */
    const int16_t *imposters; /* ring [max_size][n_imposters] int16 */
    int64_t max_size;
    const int64_t *indices;   /* [n] device: the sampled ring rows (torch.randint(0, size, (batch_size,)), replay_memory.py:89) */
    int64_t n;
    double gamma;             /* DQNTeamTrainer.gamma (train.py:42-45) */
    susnet_dqn_team team[2];  /* [0] imposters, [1] crew (train.py:91-99) */
    float *losses_out;        /* [2] float32 device: the accumulated losses [imposter, crew] (train.py:60, 139) */
    void *workspace;          /* device scratch of susnet_dqn_workspace_bytes bytes, 256-byte aligned */
    uint64_t workspace_bytes;
} susnet_dqn_io;
int susnet_dqn_workspace_bytes(const susnet_env *env, const susnet_dqn_io *io, uint64_t *bytes_out);
int susnet_dqn_train_step(susnet_env *env, const susnet_dqn_io *io, void *stream);

/* A sweep's train step.  The reference's users run sweeps: notebooks/experiment_1v1.ipynb and notebooks/experiment_mlp.ipynb build a
 * list of configurations that differ in gamma ([0.99, 0.9, 0.8]) and call run_experiment(**config) for each -- the same game, the same
 * MLP, sequence_length 1 -- and every one of them runs DQNTeamTrainer.train_step (src/train.py:50-149) on its own.  At the batch sizes
 * they use one learner's step is a chain of launches of ONE workgroup each; this call runs the steps of n_learners independent
 * learners of one shape in the SAME launches (the learner is the grid's second dimension): 1 launch to split the batches, 2 per
 * (agent, enabled team) update and 1 per enabled team for the packed images, whatever n_learners is, all on `stream`, no host
 * synchronisation, no parallel branches: a call can be captured in a hipGraph.
 * ios[k] is a complete susnet_dqn_io as susnet_dqn_train_step takes it -- its own ring, indices, gamma, Adam constants, parameters,
 * losses_out and its own workspace of susnet_dqn_workspace_bytes(envs[k], &ios[k]) bytes -- and passes that call's checks; the handles
 * supply configuration only.  All learners agree on what the step's shape depends on: agent and imposter count, raw row size, grid and
 * feature layout, `components`, `n`, and both teams' `enabled` and `dims`.  gamma, the Adam constants, every pointer and max_size may
 * differ.  No two learners share `params` (of either team), `workspace` or `losses_out`.  Anything else returns SUSNET_E_INVALID
 * with a message naming the first offending learner and field, before anything is launched.
 * After the call every learner's params, exp_avg, exp_avg_sq, step, losses_out and packed hold BIT FOR BIT what
 * susnet_dqn_train_step(envs[k], &ios[k], stream) would have left: workgroup (g, k) does what workgroup g of that call does, and every
 * sum runs in the same order.  A learner whose (agent, team) list is empty skips that update (train.py:101) whatever the others do. */
#define SUSNET_DQN_MAX_LEARNERS 16
int susnet_dqn_train_sweep(susnet_env *const *envs, const susnet_dqn_io *ios, int32_t n_learners, void *stream);

/* The same train step -- DQNTeamTrainer.train_step (src/train.py:50-149), with exactly the semantics of susnet_dqn_train_step above:
 * agents in order, imposter team then crew team, gradients accumulating over the agents (one zero_grad per call), targets from
 * target_params with y = r on done rows, mean MSE, torch's single-tensor Adam with the step count on the device, no step for an empty
 * (agent, team) list -- for ANY served MLP stack on CALLER-SUPPLIED feature rows: every game, component set and layer stack the
 * compiled-in layouts do not know.  feat / next_feat are the FlatFeaturizer rows (susnet_featurize, FLAT mode) of the batch's states and
 * next states IN BATCH ORDER: row s belongs to indices[s]; actions, rewards, dones and imposters are read in place from the ring at
 * clamp(indices[s]).  `params` (and target_params, exp_avg, exp_avg_sq) is flat in MLP.parameters() order for 1 .. 7 Linear layers:
 * W0, b0, a0, W1, b1, a1, ..., W_last, b_last (a_l: the one-element PReLU weight behind layer l); 4-byte alignment is all that is assumed.
 *   Served: the layer stacks of susnet_mlp_forward (n_dims 2 .. 8, F = dims[0] in 1 .. SUSNET_MLP_MAX_F, hidden widths 1 .. 256,
 * n_actions = dims[n_dims-1] in 1 .. 32), one imposter, 2 .. 16 agents, n in 0 .. 2^30, both enabled teams with the same dims[0],
 * lr >= 0, 0 <= beta < 1, team[].packed == NULL (there is no image: susnet_mlp_forward reads params in place, so the next forward sees
 * the step).  Anything else: SUSNET_E_INVALID with a message that names the field, before anything is launched.  Out-of-range indices and
 * actions are clamped, as in susnet_dqn_train_step.  The handle supplies the configuration (agents, imposters) and the error conventions
 * only: it need not have its state bound.
 *   Launches: one to split the batch, then two per (agent, enabled team) update (gradient partials; sum + Adam), all on `stream`, no host
 * synchronisation, no parallel branches, no atomics: a call can be captured as a hipGraph, and every sum runs in a fixed order, so two
 * runs from equal state leave identical bytes.  float32 on v_mfma_f32_32x32x2_f32.  The gradient kernel runs at most 256 workgroups, and
 * fewer where the workgroups' partial gradients together would exceed 64 MiB. */
typedef struct susnet_mlp_train_io {
    const float *feat;        /* device [n][F] float32, contiguous, BATCH order: row s belongs to indices[s] (FlatFeaturizer rows of states) */
    const float *next_feat;   /* device [n][F]: the same of next_states */
    const int64_t *actions;   /* ring [max_size][A] int64   -- read in place at indices, as susnet_dqn_io */
    const float *rewards;     /* ring [max_size][A] float32 */
    const uint8_t *dones;     /* ring [max_size][1] bool */
    const int16_t *imposters; /* ring [max_size][n_imposters] int16 */
    int64_t max_size;
    const int64_t *indices;   /* [n] device: the sampled ring rows */
    int64_t n;
    double gamma;
    susnet_dqn_team team[2];  /* [0] imposters, [1] crew; n_dims 2 .. 8, dims = [F, h.., n_actions]; `packed` must be NULL */
    float *losses_out;        /* [2] float32 device: the accumulated losses [imposter, crew] */
    void *workspace;          /* device scratch of susnet_mlp_train_workspace_bytes bytes, 256-byte aligned */
    uint64_t workspace_bytes;
} susnet_mlp_train_io;
int susnet_mlp_train_workspace_bytes(const susnet_env *env, const susnet_mlp_train_io *io, uint64_t *bytes_out);
int susnet_mlp_train_step(susnet_env *env, const susnet_mlp_train_io *io, void *stream);

/* A sweep's dense train step: what susnet_dqn_train_sweep does for the fused learner, for susnet_mlp_train_step.  The reference's sweeps
 * (notebooks/experiment_mlp.ipynb: `for config in configs: run_experiment(**config)` over gamma on ImposterTrainingGround with four feature
 * sets, [F, 256, 128, 64, 16, n_actions]; every MLP run at the default sequence_length 2) mostly lie off the compiled-in layouts, so each
 * run's DQNTeamTrainer.train_step (src/train.py:50-149) is the dense step: at the reference's batch of 32 rows a chain of
 * 1 + 2 x agents x enabled teams launches in which one workgroup works.  This call runs the steps of n_learners independent learners of
 * one shape in the SAME launches, the learner being the grid's second dimension.
 *   ios[k] is a complete susnet_mlp_train_io as susnet_mlp_train_step takes it -- its own feature rows, ring pointers, indices, gamma,
 * Adam constants, parameters, losses_out and its own workspace of susnet_mlp_train_workspace_bytes(envs[k], &ios[k]) bytes -- and passes
 * every check of that call (the same plan and pointer checks run per learner; a learner's own message is carried through behind
 * "learner k: ").  The handles supply configuration only.
 *   Served: 1 .. SUSNET_MLP_SWEEP_MAX_LEARNERS learners, each one served by the single call, that AGREE on what shapes the step: agent and
 * imposter count, n, both teams' `enabled` and the enabled teams' n_dims / dims -- hence on the grid and on the workspace layout.  gamma,
 * the Adam constants, max_size and every pointer may differ.  No two learners share `params` (of either team), `workspace` or
 * `losses_out`.  A learner's record (the pointers that differ and gamma, 128 bytes) times 16 and one network description fit the 4 KB of a
 * launch's arguments: the records travel by value, there is no table argument.  Anything else: SUSNET_E_INVALID before anything is
 * launched, the message naming the entry point, the first offending learner and the field ("susnet_mlp_train_sweep: learner 1:
 * team[0].dims differs from learner 0's ..").
 *   After the call every learner's params, exp_avg, exp_avg_sq, step (of either team) and losses_out hold BIT FOR BIT what its own
 * susnet_mlp_train_step(envs[k], &ios[k], stream) would have left: workgroup (g, k) walks the tiles workgroup g of that call walks, in the
 * same order, into the same partial slot and pre-activation slice.  A learner whose (agent, team) list is empty skips that update
 * (train.py:101) and keeps its step count, whatever the others do.
 *   Launches: 1 to split the batches, then 2 per (agent, enabled team) update (gradient partials; the fused learner's sweep form of
 * k_train_adam over the learners): 1 + 2 x agents x enabled teams per call whatever n_learners and the data are (n == 0: the first launch
 * alone, which zeroes every learner's losses).  All on `stream`, no host synchronisation, no parallel branches, no atomics: a call can be
 * captured as a hipGraph (after one eager call, which sets the gradient kernel's LDS ceiling). */
#define SUSNET_MLP_SWEEP_MAX_LEARNERS 16
int susnet_mlp_train_sweep(susnet_env *const *envs, const susnet_mlp_train_io *ios, int32_t n_learners, void *stream);

/* The same train step once more -- DQNTeamTrainer.train_step (src/train.py:50-149) with exactly the semantics of susnet_dqn_train_step and
 * susnet_mlp_train_step above: agents in order, imposter team then crew team, gradients accumulating over the agents (one zero_grad per
 * call), y = r + gamma max_a target(s') with y = r on done rows, mean MSE, torch's single-tensor Adam with the step count on the device, no
 * step for an empty (agent, team) list, out-of-range indices and actions clamped -- for the reference's SpatialDQN (src/models/dqn.py:205-301:
 * Conv2d + ReLU stack per window step, tanh nn.RNN, PReLU head; the network susnet_spatial_forward computes) in TRAINING mode.
 *   Inputs are the featurizers' tensors of the batch's states and next states IN BATCH ORDER (row s belongs to indices[s]), addressed as
 * susnet_spatial_io addresses them, with the three (row, agent, timestep) strides: the Perspective featurizer's buffers are read in place, the
 * Global featurizer's shared planes have an agent stride of 0.  spatial and next_spatial share spatial_stride, non_spatial and
 * next_non_spatial share non_spatial_stride.  actions, rewards, dones and imposters are read in place from the ring at clamp(indices[s]).
 *   team[].params (target_params, exp_avg, exp_avg_sq likewise) is flat in SpatialDQN.parameters() order: cnn.model.{0,2,..}.weight / bias
 * ([conv_out][C_in][k][k], [conv_out]), then per RNN layer weight_ih_l [H][R or H], weight_hh_l [H][H], bias_ih_l, bias_hh_l, then the head
 * W0, b0, a0, .., W_last, b_last (as susnet_mlp_train_step); 4-byte alignment is all that is assumed.  team[].n_dims / dims describe the HEAD
 * ([rnn_hidden, h1, .., n_actions]); net[] the rest of the team's network.  team[].packed must be NULL: susnet_spatial_forward reads params in
 * place, so the next forward sees the step.
 *   Training-mode semantics: the kernels compute no dropout (nn.RNN drops out between layers only: callers serve rnn dropout == 0 or one
 * layer).  ReLU passes the gradient where its output is > 0 and nothing at exactly 0, as torch does; PReLU as susnet_mlp_train_step (z > 0 ? g :
 * a g, d slope = sum over z <= 0 of z g); tanh backward is (1 - h^2) g on the stored h; bias_ih_l and bias_hh_l receive the same gradient; the
 * non-spatial columns of the RNN input are inputs, not parameters.
 *   Served: per enabled team the networks susnet_spatial_forward serves -- T in 1 .. 8, N in 1 .. 16, C in 1 .. 32, n_conv in 1 .. 4,
 * conv_out in 1 .. 32, k in {1, 3, 5}, conv_stride 1 .. 4, conv_padding 0 .. 8, conv_dilation 1 .. 4, every layer's output size at least 1,
 * Fn >= 0, R = conv_out * H_out^2 + Fn <= SUSNET_SPATIAL_MAX_R, rnn_layers 1 .. 4, rnn_hidden 1 .. 256, the head n_dims 2 .. 8 with dims[0] ==
 * rnn_hidden, hidden widths 1 .. 256, at most 32 outputs; none of the forward's bounds is narrowed (no activation is resident in LDS beyond
 * the head's fixed buffers) --, one imposter, 2 .. 16 agents, n in 0 .. 2^30, both enabled teams with the same T, N, C and Fn (they read the
 * same inputs), lr >= 0, 0 <= beta < 1, strides >= 0, every pointer non-NULL and 4-byte aligned (Fn == 0: non_spatial / next_non_spatial may
 * be NULL), the workspace 256-byte aligned and of susnet_spatial_train_workspace_bytes bytes (it grows with n: the RNN inputs of both
 * networks and the convolutions' saved activations and their gradients, n x T images each).  Anything else: SUSNET_E_INVALID with a message
 * that names the field, before anything is launched.  The handle supplies the configuration (agents, imposters) and the error conventions only.
 *   Launches: 1 to split the batch, then 4 per (agent, enabled team) update -- 1 + 4 x agents x enabled teams per call, whatever the data:
 *     convolutions  (vector ALU) of the update's rows, online network on the states (every layer's output kept in the workspace) and TARGET
 *                   network on the next states, both RNN input rows written; the target network's Q rows are computed inside the update,
 *                   never by a launch of their own, and the target network is not updated;
 *     recurrence    target then online recurrence and head on v_mfma_f32_32x32x2_f32 over tiles of 32 rows, 2 (Q - y) / count back through
 *                   the head and through time; gradients of the head's and the RNN's parameters as the workgroup's partial, the gradient
 *                   of the RNN input's convolution columns into the workspace;
 *     convolutions' backward (vector ALU): through the ReLUs and the transposed convolutions, then every weight's sum over the
 *                   workgroup's images in a fixed order;
 *     k_train_adam  as the other two learners: partials summed in workgroup order, accumulated over the agents, Adam.
 * All on `stream`, no host synchronisation, no parallel branches, no atomics: a call can be captured as a hipGraph, and every sum runs in a
 * fixed order, so two runs from equal state leave identical bytes.  The gradient kernels run SUSNET_SPATIAL_TRAIN_MAX_GRID workgroups at
 * most, and fewer where the partial gradients together would exceed 64 MiB. */
#define SUSNET_SPATIAL_TRAIN_MAX_GRID 256
typedef struct susnet_spatial_net {
    int32_t T, N, C, Fn;             /* window steps, image size, input channels, non-spatial features per step */
    int32_t n_conv, k;               /* as susnet_spatial_io */
    int32_t conv_out[4], conv_stride[4], conv_padding[4], conv_dilation[4];
    int32_t rnn_layers, rnn_hidden;
} susnet_spatial_net;
typedef struct susnet_spatial_train_io {
    susnet_spatial_net net[2];       /* [0] imposters, [1] crew: looked at where team[].enabled */
    susnet_dqn_team team[2];         /* n_dims / dims: the head [rnn_hidden, h.., n_actions]; `packed` must be NULL */
    const float *spatial;            /* device float32, BATCH order: row s belongs to indices[s] */
    const float *next_spatial;       /* the same of next_states */
    int64_t spatial_stride[3];       /* floats: per row, per agent, per timestep; an image [C][N][N] is contiguous */
    const float *non_spatial;        /* device float32 (Fn == 0: may be NULL) */
    const float *next_non_spatial;
    int64_t non_spatial_stride[3];   /* floats: per row, per agent, per timestep; a step's Fn features are contiguous */
    const int64_t *actions;          /* ring [max_size][A] int64   -- read in place at indices, as susnet_dqn_io */
    const float *rewards;            /* ring [max_size][A] float32 */
    const uint8_t *dones;            /* ring [max_size][1] bool */
    const int16_t *imposters;        /* ring [max_size][n_imposters] int16 */
    int64_t max_size;
    const int64_t *indices;          /* [n] device: the sampled ring rows */
    int64_t n;
    double gamma;
    float *losses_out;               /* [2] float32 device: the accumulated losses [imposter, crew] */
    void *workspace;                 /* device scratch of susnet_spatial_train_workspace_bytes bytes, 256-byte aligned */
    uint64_t workspace_bytes;
} susnet_spatial_train_io;
int susnet_spatial_train_workspace_bytes(const susnet_env *env, const susnet_spatial_train_io *io, uint64_t *bytes_out);
int susnet_spatial_train_step(susnet_env *env, const susnet_spatial_train_io *io, void *stream);

/* Dropout between the layers of the SpatialDQN's nn.RNN in the TRAIN STEP (training mode, rnn_dropout = p > 0, rnn_layers = L > 1), opt-in:
 * the entry points below.  susnet_spatial_train_step and its kernels are as they were (no dropout); susnet_spatial_forward stays the
 * EVAL-mode forward, and susnet_spatial_forward_dropout (further down) is its training-mode form: the reference never calls eval(), so
 * its agents ACT under this dropout too (train.py:104, 355-381).
 *   What torch computes (nn.RNN, batch_first, training): the output sequence of every layer l < L - 1 is multiplied elementwise by a mask m_l of
 * values 0 (probability p) and 1 / (1 - p), and the product feeds layer l + 1 ONLY: layer l's own recurrence W_hh h_l[t-1] reads the
 * undropped h_l, and the last layer's output -- what the head reads -- is not dropped.  torch's mask stream cannot be reproduced on the
 * device (and its own CPU and GPU streams differ), so parity is "equal given equal masks", and the library hands its masks out:
 * susnet_rnn_dropout_mask.
 *   The mask.  m(net, agent, row, t, layer, unit) is 0 or s = 1.0f / (1.0f - p) in float32, a pure function of its eight inputs (seed and
 * offset besides those six) -- never of the grid, the tile, the wave or the order of a list.  One Philox4x32-10 block per four consecutive
 * units, G = row_base + row:
 *     key      = (seed & 0xffffffff, seed >> 32)
 *     counter  = (unit / 4 | layer << 8 | t << 12 | net << 16 | agent << 20,  G & 0xffffffff,  (G >> 32) & 0xff | (offset >> 32) << 8,
 *                 offset & 0xffffffff)
 *     word j of the block (j = 0 .. 3, the order of the counter words after the ten rounds) belongs to unit 4 (unit / 4) + j;
 *     the element is KEPT (m = s) iff word >= floor(p * 2^32), computed in float64 from the float32 p; floor(p * 2^32) == 0
 *     (p == 0, or a positive p below 2^-32) keeps everything with m = 1.0f.
 *   net: 0 the online network, 1 the target network.  layer: the layer whose OUTPUT is masked, 0 .. L - 2.  agent = the update's agent,
 * row = the position s in the sampled batch (not the slot in the (agent, team) list).  A caller advances `offset` between calls that must
 * not repeat their masks (a captured graph replays its masks: capture is the caller's decision).  Refused (SUSNET_E_INVALID, the field
 * named, before any launch): drop NULL, p outside [0, 1) or NaN, offset >= 2^56, row_base < 0 or row_base + rows > 2^40, and everything the
 * plain call refuses.
 *
 * susnet_spatial_train_step_dropout: susnet_spatial_train_step with the online network's forward and backward pass and the target
 * network's forward under their masks: forward in[l+1][t] = m[l][t] * h[l][t]; dz[l][t] = (1 - h^2) (m[l][t] * (W_ih[l+1]^T dz[l+1][t]) +
 * W_hh[l]^T dz[l][t+1] (+ the head's term)); dW_ih[l+1] += dz[l+1][t] (m[l][t] * h[l][t])^T.  drop: TWO structs, [0] imposters, [1] crew
 * (looked at where team[].enabled): drop[team].p[0] masks the online network, drop[team].p[1] the target network.  The same launch count,
 * no atomics, no host wait, bitwise reproducible for equal (state, seed, offset).  The multipliers of a tile are kept in the workspace,
 * which is therefore larger than the plain step's: susnet_spatial_train_dropout_workspace_bytes is its query (the plain query does NOT
 * serve the dropout step).  With every p of the enabled teams 0 the call runs susnet_spatial_train_step's kernels.
 * susnet_rnn_dropout_mask: the multipliers out[layers - 1][n][T][H] (device float32, 4-byte aligned) that the call above uses for the
 * same `drop`, `net` (p = drop->p[net]) and `agent`, rows row_base .. row_base + n - 1.  Served: net 0 / 1, agent 0 .. 4095, layers 2 .. 4,
 * n >= 1, T 1 .. 8, H 1 .. 256.  One launch.
 *
 * ACTING under dropout.  The mask function is the one above; an acting call with io->agents = A gives row r of its n rows the coordinates
 *     agent  = r % A
 *     row G  = drop->row_base + r / A      (the env id: a sharded batch passes its first env id as row_base)
 *     t      = the window step, layer = the masked layer (0 .. L - 2), offset = drop->offset: the caller's ACTING-TICK counter
 *     net    = 2 for the imposters' acting network, 3 for the crew's
 * Nets 0 and 1 stay the train step's online and target network, so an acting mask never coincides with a training mask of the same seed,
 * and the two teams' forwards of one tick (same offset) use different masks.
 * susnet_spatial_forward_dropout: susnet_spatial_forward with the recurrence in nn.RNN's TRAINING mode -- layer l + 1 reads
 * m[l][t] * h[l][t], layer l's own recurrence the undropped h[l][t], the head the undropped top layer; the convolutions are the plain
 * call's kernel -- with p = drop->p[net - 2] (p[0] the imposters' acting network, p[1] the crew's; the other p is not looked at).  The
 * summation orders are the plain call's; the product m * h is one float32 multiplication, made where h is written.  With p == 0,
 * floor(p * 2^32) == 0 or rnn_layers == 1 the call launches susnet_spatial_forward's kernels: the result is that call's bit for bit.
 * Otherwise the recurrence kernel is k_spatial_rnn_dropout, which keeps the products in LDS behind the hidden states: its LDS rule is
 * (rnn_layers + 2) x 64 rows x max(rnn_hidden, the head's hidden widths) floats at rnn_layers == 2 and (rnn_layers + 3) x ... from
 * rnn_layers == 3 on, within a workgroup's 160 KiB (so rnn_hidden 128 is served with up to two layers under dropout, 64 with up to four).
 * Equal (inputs, seed, offset, row_base, net) give equal bytes, whatever the grid; rows [k A, (k + m) A) of a batch forwarded alone with
 * row_base + k give those rows' bytes.  Refused (SUSNET_E_INVALID, the field named, before any launch): drop NULL, net outside 2 .. 3,
 * p outside [0, 1) or NaN, offset >= 2^56, row_base < 0 or row_base + ceil(n / agents) > 2^40, agents > 4096, the LDS rule above (the
 * bytes in the message), and everything susnet_spatial_forward refuses, with that call's messages behind this call's name.
 * susnet_spatial_act_dropout_mask: the multipliers out[layers - 1][n][T][H] (device float32, 4-byte aligned) that call applies to rows
 * 0 .. n - 1 for the same `drop`, `net` and `agents`.  Served: net 2 / 3, agents 1 .. 4096, layers 2 .. 4, n >= 1, T 1 .. 8, H 1 .. 256.
 * One launch.  (susnet_rnn_dropout_mask serves nets 0 / 1 only, as before.) */
typedef struct susnet_rnn_dropout {
    float p[2];                      /* [0] the online network, [1] the target network; 0 switches that net's mask off.  The acting
                                        calls: [0] the imposters' acting network (net 2), [1] the crew's (net 3) */
    uint64_t seed;
    uint64_t offset;                 /* below 2^56: the caller's call counter */
    int64_t row_base;                /* added to every row index */
} susnet_rnn_dropout;
int susnet_spatial_train_dropout_workspace_bytes(const susnet_env *env, const susnet_spatial_train_io *io, uint64_t *bytes_out);
int susnet_spatial_train_step_dropout(susnet_env *env, const susnet_spatial_train_io *io, const susnet_rnn_dropout *drop, void *stream);
int susnet_rnn_dropout_mask(susnet_env *env, const susnet_rnn_dropout *drop, int32_t net, int32_t agent, int32_t layers, int64_t n, int32_t T,
                            int32_t H, float *out, void *stream);
int susnet_spatial_forward_dropout(susnet_env *env, const susnet_spatial_io *io, const susnet_rnn_dropout *drop, int32_t net, void *stream);
int susnet_spatial_act_dropout_mask(susnet_env *env, const susnet_rnn_dropout *drop, int32_t net, int32_t agents, int32_t layers, int64_t n,
                                    int32_t T, int32_t H, float *out, void *stream);

/* A sweep's train step for the SpatialDQN.  The reference's users run sweeps -- notebooks/experiment_1v1.ipynb and
 * notebooks/experiment_mlp.ipynb loop `for config in configs: run_experiment(**config)` over gamma ([0.99, 0.9, 0.8]) and the learning
 * rate -- and run_experiment's default model is the SpatialDQN (src/train.py:152-176, src/models/dqn.py:205-301); every run takes
 * DQNTeamTrainer.train_step (src/train.py:50-149) on its own.  At the reference's batch size (32 rows: one tile of the recurrence kernel)
 * one learner's step is a chain of 1 + 4 x agents x enabled teams launches in which a single workgroup works; this call runs the steps of
 * n_learners independent learners of one shape in the SAME launches, the learner being the grid's second dimension -- what
 * susnet_dqn_train_sweep does for the fused MLP learner.
 *   ios[k] is a complete susnet_spatial_train_io as susnet_spatial_train_step takes it -- its own batch tensors, ring pointers, indices,
 * gamma, Adam constants, parameters, losses_out and its own workspace, of susnet_spatial_train_workspace_bytes(envs[k], &ios[k]) bytes
 * where drops == NULL and of susnet_spatial_train_dropout_workspace_bytes otherwise -- and passes every check of that call (the same plan,
 * pointer and dropout checks run per learner; a learner's own message is carried through behind "learner k: ").  The handles supply
 * configuration only.  drops == NULL: every learner takes the plain step.  Otherwise drops[2 k + team] is what
 * susnet_spatial_train_step_dropout would get as drop[team] for learner k.
 *   Served: 1 .. SUSNET_SPATIAL_SWEEP_MAX_LEARNERS learners, each one served by the single call, that AGREE on what shapes the step: agent
 * and imposter count, n, both teams' `enabled`, every field of net[] and team[].n_dims / dims of the enabled teams, the three spatial
 * strides and (Fn > 0) the three non-spatial strides, and per team whether the team is masked (a p > 0 with more than one RNN layer: it
 * selects the recurrence kernel).  gamma, the Adam constants, max_size, every pointer and the dropout seed, offset, row_base and p values
 * may differ.  No two learners share `params` (of either team), `workspace` or `losses_out`.  `table` is device scratch of
 * susnet_spatial_train_sweep_table_bytes(n_learners) bytes, 256-byte aligned: a learner's record (pointers, gamma, dropout constants,
 * about 250 bytes) times 16 and the two networks' descriptions exceed the 4 KB of a launch's arguments, so the select launches write the
 * records there from their arguments -- no copy from the host, the call stays capturable -- and the update's kernels read them through a
 * pointer; what the learners agree on (networks, strides, n, agent count, workspace offsets) is kept once.  The table carries 16 learners.
 * Anything else: SUSNET_E_INVALID before anything is launched, the message naming the entry point, the first offending learner and the
 * field ("susnet_spatial_train_sweep: learner 2: net[0].rnn_hidden differs from learner 0's ..").
 *   After the call every learner's params, exp_avg, exp_avg_sq, step (of either team) and losses_out hold BIT FOR BIT what its own
 * susnet_spatial_train_step(envs[k], &ios[k], stream) -- with drops: susnet_spatial_train_step_dropout(envs[k], &ios[k], drops + 2 k,
 * stream) -- would have left: workgroup (g, k) walks the tiles and images workgroup g of that call walks, in the same summation order, and
 * writes the same partial slot.  A learner whose (agent, team) list is empty skips that update (train.py:101) whatever the others do.
 *   Launches: S to split the batches and fill the table -- S = 1 for n_learners <= 8, S = 2 above (8 learners' records per launch) --, then
 * 4 per (agent, enabled team) update (convolutions, recurrence, convolutions' backward, and the fused learner's sweep form of k_train_adam
 * over the learners): S + 4 x agents x enabled teams per call whatever n_learners and the data are (n == 0: the S launches alone, which zero
 * every learner's losses).  All on `stream`, no host synchronisation, no parallel branches, no atomics: a call can be captured as a
 * hipGraph (after one eager call, which sets the recurrence kernels' LDS ceilings). */
#define SUSNET_SPATIAL_SWEEP_MAX_LEARNERS 16
int susnet_spatial_train_sweep_table_bytes(int32_t n_learners, uint64_t *bytes_out);
int susnet_spatial_train_sweep(susnet_env *const *envs, const susnet_spatial_train_io *ios, const susnet_rnn_dropout *drops /* [n_learners][2] or NULL */,
                               int32_t n_learners, void *table, uint64_t table_bytes, void *stream);

/* Per-episode returns and lengths from a feed block -- train()'s bookkeeping (src/train.py:385-386, 419-450) for B environments in
 * lockstep.  Inputs: the [T][B] feed arrays as susnet_qnet_policy_rollout / susnet_step write them and susnet_ring_append reads them.
 * Per tick t and environment b, for every agent: G[a] = (double)rewards[t][b][a] + gamma * G[a] in float64, the product rounded before
 * the add (no fused multiply-add: numpy makes a temporary).  Where done | truncated: one record is appended to the log with
 * imposter_return = mean of G over the agents in roles[t][b], crew_return = mean over the others -- each in numpy's summation order
 * (below 8 values left to right from 0.0; from 8 values ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)), then x8, x9, ... one by one; divided by
 * the count; an empty team gives NaN) --, length = t_episode + 1, tick = tick_base + t, env = b; then G = 0 and t_episode = 0 for that
 * environment.  Otherwise t_episode += 1.  G and t_episode are carried between calls in `carry`.
 * Log order is tick-major, env-minor -- what a host loop over ticks and environments appends -- on every run: positions come from
 * per-(tick, wave) ballot counts and a scan in fixed order, never from an atomic.  When the log is full further episodes are counted in
 * *dropped and not written; the carried state still advances.  Three launches per call whatever n_ticks and the batch are, no host
 * synchronisation: a call can be captured in a hipGraph.  Served: 2 .. 12 agents, any batch, any n_ticks >= 1.  The handle supplies
 * the configuration (agent count, batch) only; no environment state is read.
 * susnet_episode_stats_bytes: the sizes of `carry` (float64 G[A][B], then int32 t_episode[B]; all zero = every environment at the start
 * of an episode) and of `workspace` for blocks of up to n_ticks ticks. */
#define SUSNET_EPISODE_DONE 1      /* ended_by bits */
#define SUSNET_EPISODE_TRUNCATED 2
typedef struct susnet_episode_record {
    double imposter_return;   /* G[imposter_mask].mean() (train.py:421) */
    double crew_return;       /* G[~imposter_mask].mean() (train.py:422) */
    int64_t tick;             /* tick_base + t: the lockstep tick at which the episode ended */
    int32_t env;              /* b */
    int32_t length;           /* steps of the episode: the reference's t_episode + 1 (train.py:430) */
    int32_t ended_by;         /* SUSNET_EPISODE_DONE | SUSNET_EPISODE_TRUNCATED */
    int32_t reserved;         /* 0 */
} susnet_episode_record;
typedef struct susnet_episode_io {
    int32_t n_ticks;          /* T >= 1 */
    int32_t reserved;
    const float *rewards;     /* [T][B][A] float32 */
    const uint8_t *done;      /* [T][B] */
    const uint8_t *truncated; /* [T][B] */
    const uint16_t *roles;    /* [T][B] imposter bitmask of the episode that acted */
    double gamma;
    int64_t tick_base;        /* the lockstep tick index of slot 0 */
    void *carry;              /* device, carry_bytes of susnet_episode_stats_bytes, 8-byte aligned; read and updated */
    uint64_t carry_bytes;
    susnet_episode_record *log; /* device [capacity], append-only */
    int64_t capacity;
    int64_t *count;           /* device [1]: records in the log; read and advanced on the device */
    int64_t *dropped;         /* device [1]: episodes that found the log full */
    void *workspace;          /* device scratch, workspace_bytes of susnet_episode_stats_bytes for >= n_ticks, 8-byte aligned */
    uint64_t workspace_bytes;
    /* both or neither: the feed's info records and a second log parallel to `log` -- the record of every ended (tick, env) is copied to
     * info_log[pos], pos = the position of the episode's record in `log`: same count, same dropped */
    const susnet_episode_info *info; /* [T][B]: susnet_feed_io.ep_info (read where done | truncated), or NULL */
    susnet_episode_info *info_log;   /* device [capacity], 16-byte aligned, or NULL */
} susnet_episode_io;
int susnet_episode_stats_bytes(const susnet_env *env, int32_t n_ticks, uint64_t *carry_bytes_out, uint64_t *workspace_bytes_out);
int susnet_episode_stats(susnet_env *env, const susnet_episode_io *io, void *stream);

/* Synchronises `stream`, reads and clears the device error word. Returns 0 or the most severe
 * SUSNET_E_ACTION_* / SUSNET_E_TAPE / SUSNET_E_ROW code; *bits_out receives the raw bits. */
int susnet_poll_errors(susnet_env *env, uint32_t *bits_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SUSNET_H */
