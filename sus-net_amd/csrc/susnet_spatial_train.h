// susnet_spatial_train.h -- susnet_spatial_train_step: the DQN learner's train step (DQNTeamTrainer.train_step, src/train.py:50-149;
// susnet_train.h has the reference notes) for the reference SpatialDQN (src/models/dqn.py:205-301) -- the network susnet_spatial_forward
// computes (susnet_spatial.h) -- in training mode without dropout.  The kernels: inst_spatial_train.hip.
//
// Per train step, on one stream, no host synchronisation, no atomics:
//   k_sp_train_select    ONE workgroup: tr_select with batch positions in the lists, as k_mlp_train_select; it also copies the two teams'
//                        network descriptions (SpTrainNet) into the workspace, where the update's kernels read them.
//   per (agent, enabled team) update, four launches:
//   k_sp_train_conv      vector ALU, a workgroup per image (an image = one window step of one row of the update's list; grid-stride over
//                        2 count T jobs: the online network on the states, then the target network on the next states).  A layer is a loop
//                        over its outputs, one fmaf chain per output starting as the bias over (c_in, ky, kx) ascending; the online
//                        network's layer outputs go to the workspace (the backward pass reads them), the target network's ping-pong in the
//                        workgroup's own slice; the last layer writes the RNN input row, the step's non-spatial features behind it.
//   k_sp_train_rnn       v_mfma_f32_32x32x2_f32 through susnet_train_core.h's tr_mfma, a workgroup walks tiles of 32 list rows.  The
//                        recurrence of the target network, its head, max over actions -> y; the online recurrence (every h[l][t] kept in the
//                        workgroup's slice of the workspace as [unit][32]) and head (pre-activations kept as the dense learner keeps them);
//                        2 (Q - y) / count back through the head (the dense learner's scheme on the same stride-33 LDS buffers), then
//                        through time: dz[l][t] = (1 - h^2) (W_ih[l+1]^T dz[l+1][t] + W_hh[l]^T dz[l][t+1] (+ the head's at the top, last
//                        step)) into a second slice; then W_ih[0]^T dz[0][t] -- its convolution columns -- into the workspace for the
//                        convolutions' backward, and the weight gradients as products over K = T x 32 (dW_hh: (T - 1) x 32), added into the
//                        workgroup's partial by read-modify-write, one writer per word (the first tile of a workgroup stores).
//   k_sp_train_conv_bwd  vector ALU, the same grid: per image of the workgroup's share (image i of workgroup i mod G) the ReLU gate
//                        (output > 0) and the transposed convolution layer by layer, top down, the gated gradients kept in the workspace;
//                        then every weight (a thread per weight) sums gradient x input over the share's images and pixels in ascending
//                        order and is stored once.  A workgroup without an image stores zeros.
//   k_train_adam         susnet_train.h's, as it is (susnet_capi_train.hip launches it).
// The two gradient kernels write disjoint parts of the same partial: [0, oWih[0]) the convolutions, [oWih[0], P] the rest and the loss sum.
// Grid: G = min(SUSNET_SPATIAL_TRAIN_MAX_GRID, n T, 64 MiB / (4 Pp)) workgroups, at least 1, for both.
// susnet_spatial_train_step_dropout is the same step with k_sp_train_rnn_dropout in k_sp_train_rnn's place (one body text, compiled twice:
// susnet_spatial_train_rnn_body.h): both recurrences under nn.RNN's inter-layer dropout, masks from susnet_dropout.h, the multipliers of a
// tile kept in a third slice per workgroup ([l][t][unit][32], l < L - 1) behind the plain step's workspace.
// Data a workgroup hands from one thread to another through global memory is separated by a workgroup barrier (release / acquire at
// workgroup scope); nothing is ever read that another workgroup of the same launch wrote.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/susnet.h"
#include "susnet_mlp_train.h"

namespace susnet {

struct SpDrop; // susnet_dropout.h: with one (and `ms`, [G][(L - 1) T H 32] floats) the update's recurrence kernel is k_sp_train_rnn_dropout

constexpr int kStConvThreads = 256;
constexpr int kStMaxGrid = SUSNET_SPATIAL_TRAIN_MAX_GRID;
constexpr int kStConvGrid = 1024;

// one team's network: shapes and float offsets into the flat parameter buffer (SpatialDQN.parameters() order)
struct SpTrainNet {
    int32_t T, N, C, Fn, n_conv, k, L, H;
    int32_t R, Rc;                  // the RNN's input width; its convolution columns (R - Fn)
    int32_t size[5], ch[5], sz[5];  // per activation level 0 .. n_conv: image size, channels, floats (ch * size^2)
    int32_t stride[4], pad[4], dil[4];
    int32_t oCW[4], oCB[4];
    int32_t oWih[4], oWhh[4], oBih[4], oBhh[4];
    MlpTrainNet head;               // nl, d, oW / oB / oA (offsets into the SAME flat buffer), zo, Z
    int32_t aoff[4], asz;           // saved output of conv layer l < n_conv - 1 within an image's record; floats per record
    int32_t maxsz;                  // the widest activation level 1 .. n_conv
    int32_t P, Pp;
};

struct SpTrainBatch {
    const float *spatial, *next_spatial, *non_spatial, *next_non_spatial;
    int64_t sp_stride[3], ns_stride[3];
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    const int16_t *imposters;
    const int64_t *idx;
    int64_t max_size, n;
    int32_t A, n_imp;
};

// the workspace behind tr_workspace_layout's part
struct SpTrainWs {
    float *X, *Xt;       // [n T][R]: RNN input rows of the online / target network, by list slot
    float *act, *dact;   // [n T][asz]: the online convolutions' saved outputs, and their gated gradients
    float *dX;           // [n T][Rc]: gradient of the last convolution's output
    float *tact;         // [conv grid][2 maxsz]: the target network's ping-pong
    float *hs, *ds;      // [G][L T H 32]: h and dz of the recurrence
    float *zs;           // [G][head.Z]
};

// ---- a sweep (susnet_spatial_train_sweep): K learners of one shape in the launches of one, the learner is blockIdx.y ----
// k_sp_train_sweep_select / _conv / _rnn / _rnn_dropout / _conv_bwd are the kernels above with the SAME body text (the select kernel calls
// the same tr_select; the others include the same susnet_spatial_train_*_body.h), so workgroup (g, k) does what workgroup g of learner k's
// own call does -- same tiles and images, same order of every sum, same partial slot -- and a learner's results are bitwise those of
// susnet_spatial_train_step / _dropout.  What a body names as a kernel argument, the sweep form builds from the learner's table entry.
// The table lives in DEVICE memory (a learner's record is about 250 bytes: 16 of them and the two networks do not fit a 4 KB argument
// block): [SpSweepShared][SpSweepLearner x K], caller-supplied, written by the select launches from their kernel arguments (no copy from
// the host: the call stays capturable) -- kSpSweepSelLearners learners per launch, so 1 launch up to 8 learners and 2 beyond -- and read
// through a pointer by the update's kernels, which run behind them on the same stream.  What the learners agree on is kept once
// (SpSweepShared): the two networks, the strides, n, the agent count and the plan's workspace offsets.  The reduce + Adam launch is
// susnet_train.h's k_train_sweep_adam as it is: its table (pointers, Adam constants) and its net (P, Pp) describe a spatial learner.
constexpr int kSpSweepMaxLearners = SUSNET_SPATIAL_SWEEP_MAX_LEARNERS;
constexpr int kSpSweepSelLearners = 8; // learners one select launch carries in its arguments

struct SpDropArgs { // SpDrop (susnet_dropout.h) without its agent, which the update supplies
    uint32_t k0, k1, off_lo, off_hi, thr[2];
    float scale[2];
    int64_t row_base;
};
struct SpSweepShared { // what all learners of a sweep agree on
    SpTrainNet net[2];
    int64_t sp_stride[3], ns_stride[3], n;
    int32_t A, n_imp;
    uint64_t off_lists, off_counts, off_gacc[2], off_partial; // TrWorkspace
    uint64_t off_X, off_Xt, off_act, off_dact, off_dX, off_tact, off_hs, off_ds, off_zs, off_ms; // SpTrainWs, and the multipliers' slices
};
struct SpSweepLearner { // one learner's own
    const float *spatial, *next_spatial, *non_spatial, *next_non_spatial;
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    const int16_t *imposters;
    const int64_t *idx;
    int64_t max_size;
    char *workspace;
    const float *prm[2], *tgt[2];
    float *step[2];
    float *losses;
    float gamma;
    int32_t pad_;
    SpDropArgs dr[2];
};
struct SpSweepSelArgs {
    SpSweepLearner l[kSpSweepSelLearners];
};
struct SpSweepTable {
    SpSweepShared sh;
    SpSweepLearner l[kSpSweepMaxLearners]; // (the first K are written and read)
};
static_assert(sizeof(SpSweepShared) + sizeof(SpSweepSelArgs) + 64 <= 4096, "the select launch's arguments: 4 KB");
static_assert(kSpSweepMaxLearners <= 2 * kSpSweepSelLearners, "at most two select launches");
inline uint64_t sp_sweep_table_bytes(int K) { return (sizeof(SpSweepShared) + (uint64_t)K * sizeof(SpSweepLearner) + 255) / 256 * 256; }

// the select launches: learners l[0 .. K) into `table` and their batches split (1 launch for K <= kSpSweepSelLearners, else 2)
hipError_t sp_train_sweep_select_launch(const SpSweepShared &sh, const SpSweepLearner *l, int K, SpSweepTable *table, hipStream_t st);
// conv, recurrence (the dropout form iff `dropout`) and conv_bwd of one (agent, team) update for the K learners of `table`
hipError_t sp_train_sweep_update_launch(const SpSweepTable *table, int K, int agent, int team, int G, int Gconv, bool dropout, hipStream_t st);

// (nets: device, two SpTrainNet -- the select kernel writes them, the update's kernels read their team's: `net` below is a DEVICE pointer)
hipError_t sp_train_select_launch(const SpTrainBatch &b, const SpTrainNet &net0, const SpTrainNet &net1, SpTrainNet *nets, int32_t *lists,
                                  int32_t *counts, float *gacc0, float *gacc1, float *losses, hipStream_t st);
hipError_t sp_train_update_launch(const SpTrainBatch &b, const SpTrainNet *net, const SpTrainWs &ws, const float *prm, const float *tgt,
                                  const int32_t *lists, const int32_t *counts, int agent, int team, float gamma, float *partial, float *step, int G,
                                  int Gconv, hipStream_t st, const SpDrop *dr = nullptr, float *ms = nullptr);

} // namespace susnet
