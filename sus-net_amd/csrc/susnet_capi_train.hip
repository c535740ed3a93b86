// susnet_capi_train.hip -- the DQN learners of the C ABI: susnet_dqn_train_step and susnet_dqn_train_sweep (the fused learner on the
// compiled-in feature layouts; its kernels: susnet_train.h, compiled here) and susnet_mlp_train_step / susnet_mlp_train_sweep (the dense
// learner on any served stack and its sweep form; their gradient kernels: inst_mlp_train.hip) and susnet_spatial_train_step / susnet_spatial_train_sweep (the SpatialDQN learner and its sweep
// form; their kernels: inst_spatial_train.hip).  All
// carve their workspace with tr_buffers and the single learners end every update with launch_adam (this unit's k_train_adam); the dense and
// the SpatialDQN learner share their handle, Adam-constant, pointer and workspace checks (check_*, below).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "susnet_qnet.h" // QNet, QRow1 / QRow3 / QRowC: the pack kernels write susnet_qnet_pack's image
#include "susnet_dense.h" // kDnMaxHidden / kDnMaxOut: the forward's widths, which the dense learner's must equal
#include "susnet_train.h"
#include "susnet_mlp_train.h"
#include "susnet_spatial_train.h"
#include "susnet_dropout.h"
#include "susnet_host.h"

using namespace susnet;

// ---- what the learners share on the host ----
// the part of a workspace every learner lays out with tr_workspace_layout, as pointers
struct TrBuffers {
    int32_t *lists, *counts;
    float *gacc[2], *partial;
};
static TrBuffers tr_buffers(void *workspace, const TrWorkspace &w) {
    char *ws = static_cast<char *>(workspace);
    return {reinterpret_cast<int32_t *>(ws + w.off_lists), reinterpret_cast<int32_t *>(ws + w.off_counts),
            {reinterpret_cast<float *>(ws + w.off_gacc[0]), reinterpret_cast<float *>(ws + w.off_gacc[1])}, reinterpret_cast<float *>(ws + w.off_partial)};
}
// the reduce + Adam launch that ends an (agent, team) update of a single learner (NET: TrainNet, MlpTrainNet, SpTrainNet -- P and Pp)
template <class NET>
static hipError_t launch_adam(const NET &net, const TrBuffers &b, int agent, int tm, int G, const susnet_dqn_team &T, float *losses, hipStream_t st) {
    hipLaunchKernelGGL(k_train_adam, dim3((unsigned)((net.P + 1 + 255) / 256)), dim3(256), 0, st, net.P, net.Pp, b.counts, agent, tm, b.partial, G, b.gacc[tm],
                       T.params, T.exp_avg, T.exp_avg_sq, T.step, T.lr, T.beta1, T.beta2, T.eps, losses);
    return hipGetLastError();
}
// The checks the dense and the SpatialDQN learner make alike, in the same words (`bad` carries the entry point's name).  The fused learner's
// older checks (dqn_plan, dqn_check_io) have words of their own.
static int check_learner(const Refuse &bad, const susnet_env *env, int64_t n, double gamma) { // the handle and the batch
    if (env->c.n_imp != 1)
        return bad("n_imposters = " + std::to_string(env->c.n_imp) + ": one imposter is served -- the reference's train_step fails on two or more, "
                   "`(batch.imposters == agent_idx).view(-1)` (src/train.py:83) has n_imposters * N entries");
    if (env->c.A < 2 || env->c.A > 16) return bad("n_agents = " + std::to_string(env->c.A) + " (served: 2 .. 16)");
    if (n < 0 || n > (1ll << 30)) return bad("n = " + std::to_string((long long)n) + " (served: 0 .. 2^30)");
    if (!(gamma == gamma)) return bad("gamma is NaN");
    return SUSNET_OK;
}
static int check_adam(const Refuse &bad, const std::string &who, const susnet_dqn_team &T) {
    if (!(T.lr >= 0.0) || !(T.beta1 >= 0.0 && T.beta1 < 1.0) || !(T.beta2 >= 0.0 && T.beta2 < 1.0) || !(T.eps >= 0.0))
        return bad(who + "lr / beta1 / beta2 / eps (served: lr >= 0, 0 <= beta < 1, eps >= 0)");
    return SUSNET_OK;
}
static int check_workspace(const Refuse &bad, const void *workspace, uint64_t have, uint64_t need, const char *query) { // (`query` tells `need`)
    if (!workspace || have < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return bad(std::string("workspace missing, smaller than ") + query + " (" + std::to_string((unsigned long long)need) + " bytes) or not 256-byte aligned");
    return SUSNET_OK;
}
template <class IO> // (susnet_mlp_train_io, susnet_spatial_train_io: the same field names)
static int check_ring_ptrs(const Refuse &bad, const IO &io) {
    if (!io.losses_out || misaligned(io.losses_out)) return bad("losses_out is NULL or not 4-byte aligned");
    const std::pair<const char *, const void *> ring[] = {{"actions", io.actions}, {"rewards", io.rewards}, {"dones", io.dones}, {"imposters", io.imposters}};
    for (const auto &r : ring)
        if (!r.second) return bad(std::string(r.first) + " is NULL");
    if (io.max_size < 1) return bad("max_size = " + std::to_string((long long)io.max_size) + " (at least one ring row)");
    if (io.n > 0 && !io.indices) return bad("indices is NULL");
    return SUSNET_OK;
}
static int check_team_ptrs(const Refuse &bad, const susnet_dqn_team (&team)[2]) {
    for (int tm = 0; tm < 2; tm++) {
        const susnet_dqn_team &T = team[tm];
        if (!T.enabled) continue;
        const std::string who = "team[" + std::to_string(tm) + "].";
        if (!T.params || misaligned(T.params)) return bad(who + "params is NULL or not 4-byte aligned");
        if (!T.target_params || misaligned(T.target_params)) return bad(who + "target_params is NULL or not 4-byte aligned");
        if (!T.exp_avg || misaligned(T.exp_avg)) return bad(who + "exp_avg is NULL or not 4-byte aligned");
        if (!T.exp_avg_sq || misaligned(T.exp_avg_sq)) return bad(who + "exp_avg_sq is NULL or not 4-byte aligned");
        if (!T.step || misaligned(T.step)) return bad(who + "step is NULL or not 4-byte aligned");
    }
    return SUSNET_OK;
}
// what the four *_workspace_bytes entry points (`entry`: the one's name) do around their learner's plan (PLAN: its type; `plan(pl)` fills it)
template <class PLAN, class FILL>
static int plan_bytes(const char *entry, uint64_t *bytes_out, const FILL &plan) {
    PLAN pl;
    if (int rc = plan(pl)) return rc;
    if (!bytes_out) return fail(SUSNET_E_INVALID, std::string(entry) + ": null bytes_out");
    *bytes_out = pl.bytes;
    return SUSNET_OK;
}
// The checks the three sweeps make alike, in the same words: the learner count ...
static int check_n_learners(const char *entry, int32_t n_learners, int32_t most) {
    if (n_learners < 1 || n_learners > most)
        return fail(SUSNET_E_INVALID, std::string(entry) + ": n_learners " + std::to_string(n_learners) + " outside 1 .. " + std::to_string(most));
    return SUSNET_OK;
}
static std::string sweep_learner(const char *entry, int k, const std::string &what) { // (how a sweep names the learner it refuses)
    return std::string(entry) + ": learner " + std::to_string(k) + ": " + what;
}
// ... and that no two learners write the same memory (susnet_dqn_io, susnet_mlp_train_io, susnet_spatial_train_io: the same field names)
template <class IO>
static int check_learners_apart(const char *entry, const IO *ios, int K) {
    for (int k = 1; k < K; k++)
        for (int j = 0; j < k; j++) {
            const char *field = nullptr;
            if (ios[k].workspace == ios[j].workspace) field = "workspace";
            else if (ios[k].losses_out == ios[j].losses_out) field = "losses_out";
            for (int a = 0; a < 2 && !field; a++)
                for (int b = 0; b < 2 && !field; b++)
                    if (ios[k].team[a].enabled && ios[j].team[b].enabled && ios[k].team[a].params == ios[j].team[b].params)
                        field = a ? "team[1].params" : "team[0].params";
            if (field) return fail(SUSNET_E_INVALID, sweep_learner(entry, k, std::string(field) + " is shared with learner " + std::to_string(j)));
        }
    return SUSNET_OK;
}

// ---- the learner's train step (susnet_train.h) ----
struct DqnPlan : TrWorkspace {
    int feat = 0;
    TrainNet net[2];
    int64_t G = 1;
    uint64_t bytes = 0;
};
static int dqn_net(const susnet_dqn_team &tm, int feat, TrainNet &net) {
    bool ok = false;
    switch (feat) {
    case FEAT_ONEHOT: ok = qnet_dims_ok<QRow1>(tm.dims, tm.n_dims); break;
    case FEAT_ONEHOT_ALIVE_CLOSEST: ok = qnet_dims_ok<QRow3>(tm.dims, tm.n_dims); break;
    case FEAT_COORD: ok = qnet_dims_ok<QRowC>(tm.dims, tm.n_dims); break;
    }
    if (!ok || tm.dims[0] > kTrMaxF) return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: served are five Linear layers [F, <=256, <=128, <=64, <=32, <=32] on the "
                                                             "compiled-in feature layouts (those of susnet_qnet_forward)");
    for (int l = 0; l < 6; l++) net.d[l] = tm.dims[l];
    tr_param_layout(net, 5);
    return SUSNET_OK;
}
static int dqn_plan(const susnet_env *env, const susnet_dqn_io *io, DqnPlan &pl) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: null env / io");
    if (env->c.n_imp != 1)
        return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: one imposter is served -- the reference's train_step fails on two or more, "
                                      "`(batch.imposters == agent_idx).view(-1)` (src/train.py:83) has n_imposters * N entries");
    if (io->trajectory_size != 1) return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: trajectory_size 1 is served (MLP on one state)");
    if (io->n < 0 || io->n > (1ll << 30)) return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: n out of range");
    if (io->n_components < 1 || io->n_components > 16) return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: n_components");
    pl.feat = qnet_feat(env, io->components, io->n_components);
    if (!pl.feat) return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: the feature layout has no compiled-in writer");
    int64_t pmax = 4;
    for (int tm = 0; tm < 2; tm++) {
        pl.net[tm] = TrainNet{};
        if (!io->team[tm].enabled) continue;
        if (int rc = dqn_net(io->team[tm], pl.feat, pl.net[tm])) return rc;
        pmax = std::max<int64_t>(pmax, pl.net[tm].Pp);
    }
    const int64_t tiles = (io->n + kTrTS - 1) / kTrTS;
    pl.G = std::max<int64_t>(1, std::min<int64_t>(kTrMaxGrid, tiles));
    pl.bytes = tr_workspace_layout(pl, env->c.A, io->n, pl.net[0].Pp, pl.net[1].Pp, pl.G, pmax);
    return SUSNET_OK;
}

extern "C" int susnet_dqn_workspace_bytes(const susnet_env *env, const susnet_dqn_io *io, uint64_t *bytes_out) {
    return plan_bytes<DqnPlan>("susnet_dqn_workspace_bytes", bytes_out, [&](DqnPlan &pl) { return dqn_plan(env, io, pl); });
}

template <class ROW>
static int dqn_launch(const susnet_env *env, const susnet_dqn_io *io, const DqnPlan &pl, hipStream_t st) {
    static LdsOptIn opted; // the dynamic-LDS ceiling of this instantiation's kernel, once per device (susnet_host.h)
    HIP_TRY(lds_opt_in(reinterpret_cast<const void *>(&k_train_grad<ROW>), kTrLdsBytes, opted));
    const TrBuffers b = tr_buffers(io->workspace, pl);
    TrainRing ring{io->states, io->next_states, io->actions, io->rewards, io->dones, io->imposters, io->max_size,
                   (int32_t)env->layout.obs_raw_size, (int32_t)env->c.A, (int32_t)env->c.n_imp};
    const int64_t N = io->n;
    hipLaunchKernelGGL(k_train_select, dim3(1), dim3(kTrThreads), kTrThreads * 4, st, ring, io->indices, N, b.lists, b.counts, b.gacc[0], pl.net[0].P,
                       b.gacc[1], pl.net[1].P, io->losses_out);
    HIP_TRY(hipGetLastError());
    if (N == 0) return SUSNET_OK;
    for (int agent = 0; agent < env->c.A; agent++)
        for (int tm = 0; tm < 2; tm++) { // imposter team, then crew team (train.py:91-99)
            const susnet_dqn_team &T = io->team[tm];
            if (!T.enabled) continue;
            hipLaunchKernelGGL(k_train_grad<ROW>, dim3((unsigned)pl.G), dim3(kTrThreads), kTrLdsBytes, st, ring, pl.net[tm], T.params, T.target_params, b.lists,
                               b.counts, N, agent, tm, (float)io->gamma, b.partial, T.step);
            HIP_TRY(hipGetLastError());
            HIP_TRY(launch_adam(pl.net[tm], b, agent, tm, (int)pl.G, T, io->losses_out, st));
        }
    for (int tm = 0; tm < 2; tm++) {
        const susnet_dqn_team &T = io->team[tm];
        if (!T.enabled || !T.packed) continue;
        hipLaunchKernelGGL(k_train_pack<ROW>, dim3((unsigned)((QNet<ROW>::kPacked + 255) / 256)), dim3(256), 0, st, pl.net[tm], T.params, T.packed);
        HIP_TRY(hipGetLastError());
    }
    return SUSNET_OK;
}

// what susnet_dqn_train_step requires of one io beyond dqn_plan (the sweep asks the same of every learner)
static int dqn_check_io(const susnet_dqn_io *io, const DqnPlan &pl) {
    if (!io->workspace || io->workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(io->workspace) & 255u))
        return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: workspace missing, smaller than susnet_dqn_workspace_bytes or not 256-byte aligned");
    if (!io->states || !io->next_states || !io->actions || !io->rewards || !io->dones || !io->imposters || !io->losses_out || io->max_size < 1 ||
        (io->n > 0 && !io->indices))
        return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: null ring tensor / indices / losses_out");
    for (int tm = 0; tm < 2; tm++) {
        const susnet_dqn_team &T = io->team[tm];
        if (T.enabled && (!T.params || !T.target_params || !T.exp_avg || !T.exp_avg_sq || !T.step))
            return fail(SUSNET_E_INVALID, "susnet_dqn_train_step: an enabled team needs params / target_params / exp_avg / exp_avg_sq / step");
    }
    return SUSNET_OK;
}

extern "C" int susnet_dqn_train_step(susnet_env *env, const susnet_dqn_io *io, void *stream) {
    if (int rc = check_bound(env)) return rc;
    DqnPlan pl;
    if (int rc = dqn_plan(env, io, pl)) return rc;
    if (int rc = dqn_check_io(io, pl)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (pl.feat) {
    case FEAT_ONEHOT: return dqn_launch<QRow1>(env, io, pl, st);
    case FEAT_COORD: return dqn_launch<QRowC>(env, io, pl, st);
    default: return dqn_launch<QRow3>(env, io, pl, st);
    }
}

// ---- a sweep's train step: K learners in the launches of one (susnet_train.h, k_train_sweep_*) ----
template <class ROW>
static int dqn_sweep_launch(susnet_env *const *envs, const susnet_dqn_io *ios, int K, const DqnPlan *pls, hipStream_t st) {
    static LdsOptIn opted; // (as dqn_launch)
    HIP_TRY(lds_opt_in(reinterpret_cast<const void *>(&k_train_sweep_grad<ROW>), kTrLdsBytes, opted));
    const susnet_env *env = envs[0];
    const DqnPlan &pl = pls[0]; // dims, n and the agent count agree: every learner has this grid and these nets
    const int64_t N = ios[0].n;
    TrainSelTable sel{};
    TrainTable tab[2] = {};
    bool packs[2] = {false, false};
    for (int k = 0; k < K; k++) {
        const susnet_dqn_io &io = ios[k];
        const TrBuffers b = tr_buffers(io.workspace, pls[k]);
        const TrainRing ring{io.states, io.next_states, io.actions, io.rewards, io.dones, io.imposters, io.max_size,
                             (int32_t)envs[k]->layout.obs_raw_size, (int32_t)envs[k]->c.A, (int32_t)envs[k]->c.n_imp};
        sel.l[k] = TrainSelLearner{ring, io.indices, b.lists, b.counts, b.gacc[0], b.gacc[1], io.losses_out};
        for (int tm = 0; tm < 2; tm++) {
            const susnet_dqn_team &T = io.team[tm];
            if (!T.enabled) continue;
            tab[tm].l[k] = TrainLearner{ring, T.params, T.target_params, T.exp_avg, T.exp_avg_sq, T.step, b.lists, b.counts, b.gacc[tm], b.partial, io.losses_out, T.packed,
                                        T.lr, T.beta1, T.beta2, T.eps, (float)io.gamma, 0};
            packs[tm] = packs[tm] || T.packed != nullptr;
        }
    }
    const unsigned Ku = (unsigned)K;
    hipLaunchKernelGGL(k_train_sweep_select, dim3(1, Ku), dim3(kTrThreads), kTrThreads * 4, st, sel, N, pl.net[0].P, pl.net[1].P);
    HIP_TRY(hipGetLastError());
    if (N == 0) return SUSNET_OK;
    for (int agent = 0; agent < env->c.A; agent++)
        for (int tm = 0; tm < 2; tm++) { // imposter team, then crew team (train.py:91-99)
            if (!ios[0].team[tm].enabled) continue;
            hipLaunchKernelGGL(k_train_sweep_grad<ROW>, dim3((unsigned)pl.G, Ku), dim3(kTrThreads), kTrLdsBytes, st, tab[tm], pl.net[tm], N, agent, tm);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_train_sweep_adam, dim3((unsigned)((pl.net[tm].P + 1 + 255) / 256), Ku), dim3(256), 0, st, tab[tm], pl.net[tm], agent, tm,
                               (int)pl.G);
            HIP_TRY(hipGetLastError());
        }
    for (int tm = 0; tm < 2; tm++) {
        if (!ios[0].team[tm].enabled || !packs[tm]) continue;
        hipLaunchKernelGGL(k_train_sweep_pack<ROW>, dim3((unsigned)((QNet<ROW>::kPacked + 255) / 256), Ku), dim3(256), 0, st, tab[tm], pl.net[tm]);
        HIP_TRY(hipGetLastError());
    }
    return SUSNET_OK;
}

extern "C" int susnet_dqn_train_sweep(susnet_env *const *envs, const susnet_dqn_io *ios, int32_t n_learners, void *stream) {
    if (!envs || !ios) return fail(SUSNET_E_INVALID, "susnet_dqn_train_sweep: null envs / ios");
    if (int rc = check_n_learners("susnet_dqn_train_sweep", n_learners, SUSNET_DQN_MAX_LEARNERS)) return rc;
    const int K = n_learners;
    const auto who = [](int k, const std::string &what) { return sweep_learner("susnet_dqn_train_sweep", k, what); };
    DqnPlan pls[SUSNET_DQN_MAX_LEARNERS];
    for (int k = 0; k < K; k++) { // each learner passes susnet_dqn_train_step's checks ...
        int rc = check_bound(envs[k]);
        if (!rc) rc = dqn_plan(envs[k], &ios[k], pls[k]);
        if (!rc) rc = dqn_check_io(&ios[k], pls[k]);
        if (rc) return fail(rc, who(k, g_err));
    }
    const susnet_env *e0 = envs[0];
    const susnet_dqn_io &i0 = ios[0];
    for (int k = 1; k < K; k++) { // ... and all agree on what shapes the step
        const susnet_env *e = envs[k];
        const susnet_dqn_io &io = ios[k];
        const char *field = nullptr;
        if (e->c.A != e0->c.A || e->c.n_imp != e0->c.n_imp) field = "agent count";
        else if (e->layout.obs_raw_size != e0->layout.obs_raw_size) field = "raw row size";
        else if (e->c.N != e0->c.N || memcmp(e->c.grid_rows, e0->c.grid_rows, sizeof(e0->c.grid_rows)) != 0) field = "grid";
        else if (io.n_components != i0.n_components || memcmp(io.components, i0.components, sizeof(int32_t) * (size_t)i0.n_components) != 0)
            field = "components";
        else if (pls[k].feat != pls[0].feat) field = "feature layout";
        else if (io.n != i0.n) field = "n";
        for (int tm = 0; tm < 2 && !field; tm++) {
            if ((io.team[tm].enabled != 0) != (i0.team[tm].enabled != 0)) field = tm ? "team[1].enabled" : "team[0].enabled";
            else if (io.team[tm].enabled && (io.team[tm].n_dims != i0.team[tm].n_dims || memcmp(io.team[tm].dims, i0.team[tm].dims, sizeof(int32_t) * 6) != 0))
                field = tm ? "team[1].dims" : "team[0].dims";
        }
        if (field) return fail(SUSNET_E_INVALID, who(k, std::string(field) + " differs from learner 0's (a sweep runs learners of one shape)"));
    }
    if (int rc = check_learners_apart("susnet_dqn_train_sweep", ios, K)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (pls[0].feat) {
    case FEAT_ONEHOT: return dqn_sweep_launch<QRow1>(envs, ios, K, pls, st);
    case FEAT_COORD: return dqn_sweep_launch<QRowC>(envs, ios, K, pls, st);
    default: return dqn_sweep_launch<QRow3>(envs, ios, K, pls, st);
    }
}

// ---- the dense learner's train step (susnet_mlp_train.h; the kernels: inst_mlp_train.hip) ----
struct MlpTrainPlan : TrWorkspace {
    MlpTrainNet net[2];
    int64_t G = 1;
    uint64_t off_z = 0, bytes = 0;
};
static int mlp_train_plan(const susnet_env *env, const susnet_mlp_train_io *io, MlpTrainPlan &pl) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_mlp_train_step: null env / io");
    static_assert(kMtMaxHidden == kDnMaxHidden && kMtMaxOut == kDnMaxOut, "the dense learner trains what the dense forward serves"); // (one check_stack_dims)
    const Refuse bad{env, "susnet_mlp_train_step"};
    if (int rc = check_learner(bad, env, io->n, io->gamma)) return rc;
    int64_t pmax = 4, zmax = 0;
    int F = 0;
    for (int tm = 0; tm < 2; tm++) {
        pl.net[tm] = MlpTrainNet{};
        const susnet_dqn_team &T = io->team[tm];
        if (!T.enabled) continue;
        const std::string who = "team[" + std::to_string(tm) + "].";
        if (int rc = check_stack_n_dims(bad, who, T.n_dims)) return rc;
        if (int rc = check_feature_width(bad, who, T.dims[0])) return rc;
        if (int rc = check_stack_dims(bad, who, T.n_dims, T.dims, kMtMaxHidden, kMtMaxOut)) return rc;
        const int nl = T.n_dims - 1;
        if (F && T.dims[0] != F)
            return bad(who + "dims[0] = " + std::to_string(T.dims[0]) + " but team[0].dims[0] = " + std::to_string(F) + ": both teams read the same feature rows");
        F = T.dims[0];
        if (T.packed) return bad(who + "packed must be NULL (the dense forward reads params in place: there is no image to rewrite)");
        if (int rc = check_adam(bad, who, T)) return rc;
        MlpTrainNet &net = pl.net[tm];
        net.nl = nl;
        for (int l = 0; l <= nl; l++) net.d[l] = T.dims[l];
        tr_param_layout(net, nl);
        for (int l = 0; l < nl - 1; l++) { // the hidden layers' saved pre-activations, [unit][32] each
            net.zo[l] = net.Z;
            net.Z += net.d[l + 1] * kTrTS;
        }
        pmax = std::max<int64_t>(pmax, net.Pp);
        zmax = std::max<int64_t>(zmax, net.Z);
    }
    const int64_t tiles = (io->n + kTrTS - 1) / kTrTS;
    pl.G = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kMtMaxGrid, tiles), (int64_t)(kMtMaxPartialBytes / (4ull * (uint64_t)pmax))));
    pl.off_z = tr_workspace_layout(pl, env->c.A, io->n, pl.net[0].Pp, pl.net[1].Pp, pl.G, pmax);
    pl.bytes = up(pl.off_z + 4ull * (uint64_t)pl.G * (uint64_t)std::max<int64_t>(zmax, 4), 256);
    return SUSNET_OK;
}

extern "C" int susnet_mlp_train_workspace_bytes(const susnet_env *env, const susnet_mlp_train_io *io, uint64_t *bytes_out) {
    return plan_bytes<MlpTrainPlan>("susnet_mlp_train_workspace_bytes", bytes_out, [&](MlpTrainPlan &pl) { return mlp_train_plan(env, io, pl); });
}

// the checks of one call, shared with the sweep, which asks them of every learner: the plan, the workspace and every pointer
static int mlp_train_check(const susnet_env *env, const susnet_mlp_train_io *io, MlpTrainPlan &pl) {
    if (int rc = mlp_train_plan(env, io, pl)) return rc;
    const Refuse bad{env, "susnet_mlp_train_step"};
    if (int rc = check_workspace(bad, io->workspace, io->workspace_bytes, pl.bytes, "susnet_mlp_train_workspace_bytes")) return rc;
    if (int rc = check_ring_ptrs(bad, *io)) return rc;
    if (io->n > 0) {
        if (!io->feat || misaligned(io->feat)) return bad("feat is NULL or not 4-byte aligned");
        if (!io->next_feat || misaligned(io->next_feat)) return bad("next_feat is NULL or not 4-byte aligned");
    }
    return check_team_ptrs(bad, io->team);
}
// everything is checked here, before the first launch; the handle gives the configuration (A, n_imposters) and the error conventions only
extern "C" int susnet_mlp_train_step(susnet_env *env, const susnet_mlp_train_io *io, void *stream) {
    MlpTrainPlan pl;
    if (int rc = mlp_train_check(env, io, pl)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TrBuffers w = tr_buffers(io->workspace, pl);
    float *zsave = reinterpret_cast<float *>(static_cast<char *>(io->workspace) + pl.off_z);
    const MlpTrainBatch b{io->feat, io->next_feat, io->actions, io->rewards, io->dones, io->imposters, io->indices, io->max_size, io->n,
                          (int32_t)env->c.A, (int32_t)env->c.n_imp};
    HIP_TRY(mlp_train_select_launch(b, w.lists, w.counts, w.gacc[0], pl.net[0].P, w.gacc[1], pl.net[1].P, io->losses_out, st));
    if (io->n == 0) return SUSNET_OK;
    for (int agent = 0; agent < env->c.A; agent++)
        for (int tm = 0; tm < 2; tm++) { // imposter team, then crew team (train.py:91-99)
            const susnet_dqn_team &T = io->team[tm];
            if (!T.enabled) continue;
            HIP_TRY(mlp_train_grad_launch(b, pl.net[tm], T.params, T.target_params, w.lists, w.counts, agent, tm, (float)io->gamma, w.partial, zsave,
                                          T.step, (int)pl.G, st));
            HIP_TRY(launch_adam(pl.net[tm], w, agent, tm, (int)pl.G, T, io->losses_out, st));
        }
    return SUSNET_OK;
}

// ---- a sweep's dense train step: K learners in the launches of one (susnet_mlp_train.h, k_mlp_train_sweep_*) ----
static_assert(kMtSweepMaxLearners <= kTrMaxLearners, "the reduce + Adam launch is k_train_sweep_adam: its table carries the learners");

extern "C" int susnet_mlp_train_sweep(susnet_env *const *envs, const susnet_mlp_train_io *ios, int32_t n_learners, void *stream) {
    if (!envs || !ios) return fail(SUSNET_E_INVALID, "susnet_mlp_train_sweep: null envs / ios");
    if (int rc = check_n_learners("susnet_mlp_train_sweep", n_learners, SUSNET_MLP_SWEEP_MAX_LEARNERS)) return rc;
    const int K = n_learners;
    const auto who = [](int k, const std::string &what) { return sweep_learner("susnet_mlp_train_sweep", k, what); };
    std::vector<MlpTrainPlan> pls((size_t)K);
    for (int k = 0; k < K; k++) { // each learner passes susnet_mlp_train_step's checks ...
        if (!envs[k]) return fail(SUSNET_E_INVALID, who(k, "null handle"));
        if (int rc = mlp_train_check(envs[k], &ios[k], pls[(size_t)k])) return fail(rc, who(k, g_err));
    }
    const susnet_env *e0 = envs[0];
    const susnet_mlp_train_io &i0 = ios[0];
    const MlpTrainPlan &pl = pls[0];
    for (int k = 1; k < K; k++) { // ... and all agree on what shapes the step
        const susnet_env *e = envs[k];
        const susnet_mlp_train_io &io = ios[k];
        std::string field;
        if (e->c.A != e0->c.A || e->c.n_imp != e0->c.n_imp) field = "agent count";
        else if (io.n != i0.n) field = "n";
        for (int tm = 0; tm < 2 && field.empty(); tm++)
            if ((io.team[tm].enabled != 0) != (i0.team[tm].enabled != 0)) field = "team[" + std::to_string(tm) + "].enabled";
        for (int tm = 0; tm < 2 && field.empty(); tm++) {
            if (!i0.team[tm].enabled) continue;
            if (io.team[tm].n_dims != i0.team[tm].n_dims) field = "team[" + std::to_string(tm) + "].n_dims";
            else if (memcmp(io.team[tm].dims, i0.team[tm].dims, sizeof(int32_t) * (size_t)i0.team[tm].n_dims) != 0) field = "team[" + std::to_string(tm) + "].dims";
        }
        if (!field.empty()) return fail(SUSNET_E_INVALID, who(k, field + " differs from learner 0's (a sweep runs learners of one shape)"));
        if (pls[(size_t)k].bytes != pl.bytes || pls[(size_t)k].G != pl.G || pls[(size_t)k].off_z != pl.off_z)
            return fail(SUSNET_E_INVALID, who(k, "workspace plan differs from learner 0's"));
    }
    if (int rc = check_learners_apart("susnet_mlp_train_sweep", ios, K)) return rc;
    // each learner's own: the select launch's record, and per team the gradient launch's and the reduce + Adam launch's
    MlpSweepSelTable sel{};
    MlpSweepTable grad[2] = {};
    TrainTable adam[2] = {};
    TrainNet anet[2] = {};
    for (int tm = 0; tm < 2; tm++) anet[tm].P = pl.net[tm].P, anet[tm].Pp = pl.net[tm].Pp;
    for (int k = 0; k < K; k++) {
        const susnet_mlp_train_io &io = ios[k];
        const TrBuffers w = tr_buffers(io.workspace, pl);
        float *zsave = reinterpret_cast<float *>(static_cast<char *>(io.workspace) + pl.off_z);
        sel.l[k] = MlpSweepSelLearner{io.imposters, io.indices, io.max_size, w.lists, w.counts, w.gacc[0], w.gacc[1], io.losses_out};
        for (int tm = 0; tm < 2; tm++) {
            const susnet_dqn_team &T = io.team[tm];
            if (!T.enabled) continue;
            grad[tm].l[k] = MlpSweepLearner{io.feat, io.next_feat, io.actions, io.rewards, io.dones, io.imposters, io.indices, io.max_size, T.params,
                                            T.target_params, w.lists, w.counts, w.partial, zsave, T.step, (float)io.gamma, 0};
            adam[tm].l[k] = TrainLearner{TrainRing{}, T.params, T.target_params, T.exp_avg, T.exp_avg_sq, T.step, w.lists, w.counts, w.gacc[tm], w.partial,
                                         io.losses_out, nullptr, T.lr, T.beta1, T.beta2, T.eps, (float)io.gamma, 0};
        }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int A = (int)e0->c.A, n_imp = (int)e0->c.n_imp;
    HIP_TRY(mlp_train_sweep_select_launch(sel, K, i0.n, A, n_imp, pl.net[0].P, pl.net[1].P, st));
    if (i0.n == 0) return SUSNET_OK;
    for (int agent = 0; agent < A; agent++)
        for (int tm = 0; tm < 2; tm++) { // imposter team, then crew team (train.py:91-99)
            if (!i0.team[tm].enabled) continue;
            HIP_TRY(mlp_train_sweep_grad_launch(grad[tm], K, pl.net[tm], i0.n, A, n_imp, agent, tm, (int)pl.G, st));
            hipLaunchKernelGGL(k_train_sweep_adam, dim3((unsigned)((pl.net[tm].P + 1 + 255) / 256), (unsigned)K), dim3(256), 0, st, adam[tm], anet[tm], agent, tm,
                               (int)pl.G);
            HIP_TRY(hipGetLastError());
        }
    return SUSNET_OK;
}

// ---- the SpatialDQN learner's train step (susnet_spatial_train.h; the kernels: inst_spatial_train.hip) ----
struct SpTrainPlan : TrWorkspace {
    SpTrainNet net[2];
    int64_t G = 1, Gconv = 1;
    uint64_t off_X = 0, off_Xt = 0, off_act = 0, off_dact = 0, off_dX = 0, off_tact = 0, off_hs = 0, off_ds = 0, off_zs = 0, off_nets = 0, off_ms = 0, bytes = 0;
};
// one enabled team's network: the rules are check_spatial_net's (susnet_host.h, shared with susnet_spatial_forward); its own are the flat
// parameter offsets (SpatialDQN.parameters() order) and the layout of the saved activations
static int sp_train_net(const Refuse &bad, int t, const susnet_spatial_net &sn, const susnet_dqn_team &tm, SpTrainNet &net) {
    const std::string who = "net[" + std::to_string(t) + "].", team = "team[" + std::to_string(t) + "]."; // where the spatial fields and the head's sit
    SpatialGeom g;
    if (int rc = check_spatial_net(bad, who, team, sn, tm.n_dims, tm.dims, kMtMaxHidden, kMtMaxOut, g)) return rc;
    if (tm.packed) return bad(team + "packed must be NULL (susnet_spatial_forward reads params in place: there is no image to rewrite)");
    if (int rc = check_adam(bad, team, tm)) return rc;
    net = SpTrainNet{};
    net.T = sn.T, net.N = sn.N, net.C = sn.C, net.Fn = sn.Fn, net.n_conv = sn.n_conv, net.k = sn.k;
    net.R = g.R, net.Rc = g.Rc, net.L = sn.rnn_layers, net.H = sn.rnn_hidden;
    for (int l = 0; l <= sn.n_conv; l++) net.size[l] = g.size[l], net.ch[l] = g.ch[l], net.sz[l] = g.sz[l];
    int off = 0;
    const auto take = [&](int32_t &at, int floats) { at = off, off += floats; };
    for (int l = 0; l < sn.n_conv; l++) {
        net.stride[l] = sn.conv_stride[l], net.pad[l] = sn.conv_padding[l], net.dil[l] = sn.conv_dilation[l];
        take(net.oCW[l], net.ch[l + 1] * net.ch[l] * sn.k * sn.k);
        take(net.oCB[l], net.ch[l + 1]);
        net.maxsz = std::max(net.maxsz, net.sz[l + 1]);
        if (l < sn.n_conv - 1) {
            net.aoff[l] = net.asz;
            net.asz += net.sz[l + 1];
        }
    }
    for (int l = 0; l < net.L; l++) {
        take(net.oWih[l], net.H * (l == 0 ? net.R : net.H));
        take(net.oWhh[l], net.H * net.H);
        take(net.oBih[l], net.H);
        take(net.oBhh[l], net.H);
    }
    MlpTrainNet &hd = net.head;
    hd.nl = tm.n_dims - 1;
    for (int l = 0; l <= hd.nl; l++) hd.d[l] = tm.dims[l];
    tr_param_layout(hd, hd.nl);
    for (int l = 0; l < hd.nl; l++) hd.oW[l] += off, hd.oB[l] += off;
    for (int l = 0; l < hd.nl - 1; l++) {
        hd.oA[l] += off;
        hd.zo[l] = hd.Z;
        hd.Z += hd.d[l + 1] * kTrTS;
    }
    net.P = off + hd.P;
    net.Pp = (net.P + 1 + 3) / 4 * 4;
    return SUSNET_OK;
}
// `dropout`: the plan of susnet_spatial_train_step_dropout (`entry` its name) -- the multipliers' slices behind everything else
static int sp_train_plan(const susnet_env *env, const susnet_spatial_train_io *io, SpTrainPlan &pl, bool dropout = false,
                         const char *entry = "susnet_spatial_train_step") {
    if (!env || !io) return fail(SUSNET_E_INVALID, std::string(entry) + ": null env / io");
    const Refuse bad{env, entry};
    const auto S = [](long long v) { return std::to_string(v); };
    if (int rc = check_learner(bad, env, io->n, io->gamma)) return rc;
    int64_t pmax = 4, T = 1, R = 1, Rc = 1, asz = 0, maxsz = 1, slice = 1, mslice = 1, Z = 4;
    int first = -1;
    for (int tm = 0; tm < 2; tm++) {
        pl.net[tm] = SpTrainNet{};
        if (!io->team[tm].enabled) continue;
        const std::string who = "net[" + S(tm) + "].";
        if (int rc = sp_train_net(bad, tm, io->net[tm], io->team[tm], pl.net[tm])) return rc;
        const SpTrainNet &net = pl.net[tm];
        if (first >= 0) {
            const susnet_spatial_net &a = io->net[first], &c = io->net[tm];
            const char *field = a.T != c.T ? "T" : a.N != c.N ? "N" : a.C != c.C ? "C" : a.Fn != c.Fn ? "Fn" : nullptr;
            if (field) return bad(who + field + " differs from net[" + S(first) + "]." + field + ": both teams read the same inputs");
        } else first = tm;
        pmax = std::max<int64_t>(pmax, net.Pp);
        T = net.T;
        R = std::max<int64_t>(R, net.R), Rc = std::max<int64_t>(Rc, net.Rc), asz = std::max<int64_t>(asz, net.asz);
        maxsz = std::max<int64_t>(maxsz, net.maxsz);
        slice = std::max<int64_t>(slice, (int64_t)net.L * net.T * net.H * kTrTS);
        mslice = std::max<int64_t>(mslice, (int64_t)(net.L - 1) * net.T * net.H * kTrTS);
        Z = std::max<int64_t>(Z, net.head.Z);
    }
    for (int d = 0; d < 3; d++) {
        if (io->spatial_stride[d] < 0) return bad("spatial_stride[" + S(d) + "] = " + S(io->spatial_stride[d]) + " (at least 0)");
        if (first >= 0 && io->net[first].Fn > 0 && io->non_spatial_stride[d] < 0)
            return bad("non_spatial_stride[" + S(d) + "] = " + S(io->non_spatial_stride[d]) + " (at least 0)");
    }
    const int64_t images = std::max<int64_t>(1, io->n * T);
    pl.G = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kStMaxGrid, images), (int64_t)(kMtMaxPartialBytes / (4ull * (uint64_t)pmax))));
    pl.Gconv = std::min<int64_t>(kStConvGrid, 2 * images);
    uint64_t o = tr_workspace_layout(pl, env->c.A, io->n, pl.net[0].Pp, pl.net[1].Pp, pl.G, pmax);
    const auto take = [&](uint64_t &off, uint64_t floats) {
        off = o;
        o = up(o + 4ull * std::max<uint64_t>(floats, 4), 256);
    };
    take(pl.off_X, (uint64_t)images * (uint64_t)R);
    take(pl.off_Xt, (uint64_t)images * (uint64_t)R);
    take(pl.off_act, (uint64_t)images * (uint64_t)asz);
    take(pl.off_dact, (uint64_t)images * (uint64_t)asz);
    take(pl.off_dX, (uint64_t)images * (uint64_t)Rc);
    take(pl.off_tact, (uint64_t)pl.Gconv * 2ull * (uint64_t)maxsz);
    take(pl.off_hs, (uint64_t)pl.G * (uint64_t)slice);
    take(pl.off_ds, (uint64_t)pl.G * (uint64_t)slice);
    take(pl.off_zs, (uint64_t)pl.G * (uint64_t)Z);
    take(pl.off_nets, 2 * (sizeof(SpTrainNet) + 3) / 4);
    if (dropout) take(pl.off_ms, (uint64_t)pl.G * (uint64_t)mslice);
    pl.bytes = o;
    return SUSNET_OK;
}

extern "C" int susnet_spatial_train_workspace_bytes(const susnet_env *env, const susnet_spatial_train_io *io, uint64_t *bytes_out) {
    return plan_bytes<SpTrainPlan>("susnet_spatial_train_workspace_bytes", bytes_out, [&](SpTrainPlan &pl) { return sp_train_plan(env, io, pl); });
}
extern "C" int susnet_spatial_train_dropout_workspace_bytes(const susnet_env *env, const susnet_spatial_train_io *io, uint64_t *bytes_out) {
    return plan_bytes<SpTrainPlan>("susnet_spatial_train_dropout_workspace_bytes", bytes_out,
                                   [&](SpTrainPlan &pl) { return sp_train_plan(env, io, pl, true, "susnet_spatial_train_step_dropout"); });
}

// the checks of one call (`entry`: its name), shared with the sweep, which asks them of every learner: the plan, the dropout structs, the
// workspace and every pointer
struct SpTrainChecked {
    SpTrainPlan pl;
    SpDrop dr[2] = {};
    bool masked[2] = {false, false};
    int Fn = 0;
};
static int sp_train_check(const susnet_env *env, const susnet_spatial_train_io *io, const susnet_rnn_dropout *drop, const char *entry, SpTrainChecked &c) {
    SpTrainPlan &pl = c.pl;
    if (int rc = sp_train_plan(env, io, pl, drop != nullptr, entry)) return rc;
    const Refuse bad{env, entry};
    SpDrop(&dr)[2] = c.dr;
    bool(&masked)[2] = c.masked;
    for (int tm = 0; drop && tm < 2; tm++) {
        if (!io->team[tm].enabled) continue;
        if (int rc = drop_check(bad, "drop[" + std::to_string(tm) + "].", drop[tm], io->n, dr[tm])) return rc;
        masked[tm] = (dr[tm].thr[0] != 0u || dr[tm].thr[1] != 0u) && pl.net[tm].L > 1;
    }
    if (int rc = check_workspace(bad, io->workspace, io->workspace_bytes, pl.bytes,
                                 drop ? "susnet_spatial_train_dropout_workspace_bytes" : "susnet_spatial_train_workspace_bytes"))
        return rc;
    if (int rc = check_ring_ptrs(bad, *io)) return rc;
    const bool any = io->team[0].enabled || io->team[1].enabled;
    const int Fn = c.Fn = io->team[0].enabled ? io->net[0].Fn : io->team[1].enabled ? io->net[1].Fn : 0;
    if (io->n > 0 && any) {
        if (!io->spatial || misaligned(io->spatial)) return bad("spatial is NULL or not 4-byte aligned");
        if (!io->next_spatial || misaligned(io->next_spatial)) return bad("next_spatial is NULL or not 4-byte aligned");
        // (Fn = 0: nothing is read through them, so NULL is accepted, as susnet_spatial_forward does; a pointer that is given is still checked)
        if ((!io->non_spatial && Fn > 0) || misaligned(io->non_spatial)) return bad("non_spatial is NULL or not 4-byte aligned");
        if ((!io->next_non_spatial && Fn > 0) || misaligned(io->next_non_spatial)) return bad("next_non_spatial is NULL or not 4-byte aligned");
    }
    return check_team_ptrs(bad, io->team);
}
// everything is checked here, before the first launch; the handle gives the configuration (A, n_imposters) and the error conventions only.
// `drop` (susnet_spatial_train_step_dropout): two structs, [0] imposters, [1] crew; a team with a mask (a p > 0 and more than one RNN layer)
// takes k_sp_train_rnn_dropout, any other the plain kernel
static int spatial_train_step(susnet_env *env, const susnet_spatial_train_io *io, const susnet_rnn_dropout *drop, void *stream) {
    SpTrainChecked c;
    if (int rc = sp_train_check(env, io, drop, drop ? "susnet_spatial_train_step_dropout" : "susnet_spatial_train_step", c)) return rc;
    const SpTrainPlan &pl = c.pl;
    const SpDrop(&dr)[2] = c.dr;
    const bool(&masked)[2] = c.masked;
    const int Fn = c.Fn;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(io->workspace);
    const TrBuffers t = tr_buffers(io->workspace, pl);
    const auto at = [&](uint64_t off) { return reinterpret_cast<float *>(ws + off); };
    const SpTrainWs w{at(pl.off_X), at(pl.off_Xt), at(pl.off_act), at(pl.off_dact), at(pl.off_dX), at(pl.off_tact), at(pl.off_hs), at(pl.off_ds), at(pl.off_zs)};
    SpTrainBatch b{};
    b.spatial = io->spatial, b.next_spatial = io->next_spatial, b.non_spatial = io->non_spatial, b.next_non_spatial = io->next_non_spatial;
    for (int d = 0; d < 3; d++) b.sp_stride[d] = io->spatial_stride[d], b.ns_stride[d] = Fn > 0 ? io->non_spatial_stride[d] : 0;
    b.actions = io->actions, b.rewards = io->rewards, b.dones = io->dones, b.imposters = io->imposters, b.idx = io->indices;
    b.max_size = io->max_size, b.n = io->n, b.A = (int32_t)env->c.A, b.n_imp = (int32_t)env->c.n_imp;
    SpTrainNet *nets = reinterpret_cast<SpTrainNet *>(ws + pl.off_nets);
    HIP_TRY(sp_train_select_launch(b, pl.net[0], pl.net[1], nets, t.lists, t.counts, t.gacc[0], t.gacc[1], io->losses_out, st));
    if (io->n == 0) return SUSNET_OK;
    for (int agent = 0; agent < env->c.A; agent++)
        for (int tm = 0; tm < 2; tm++) { // imposter team, then crew team (train.py:91-99)
            const susnet_dqn_team &T = io->team[tm];
            if (!T.enabled) continue;
            HIP_TRY(sp_train_update_launch(b, nets + tm, w, T.params, T.target_params, t.lists, t.counts, agent, tm, (float)io->gamma, t.partial, T.step,
                                           (int)pl.G, (int)pl.Gconv, st, masked[tm] ? &dr[tm] : nullptr, masked[tm] ? at(pl.off_ms) : nullptr));
            HIP_TRY(launch_adam(pl.net[tm], t, agent, tm, (int)pl.G, T, io->losses_out, st));
        }
    return SUSNET_OK;
}
extern "C" int susnet_spatial_train_step(susnet_env *env, const susnet_spatial_train_io *io, void *stream) {
    return spatial_train_step(env, io, nullptr, stream);
}
extern "C" int susnet_spatial_train_step_dropout(susnet_env *env, const susnet_spatial_train_io *io, const susnet_rnn_dropout *drop, void *stream) {
    if (env && io && !drop) return Refuse{env, "susnet_spatial_train_step_dropout"}("drop is NULL");
    return spatial_train_step(env, io, drop, stream);
}

// ---- a sweep's SpatialDQN train step: K learners in the launches of one (susnet_spatial_train.h, k_sp_train_sweep_*) ----
static_assert(kSpSweepMaxLearners <= kTrMaxLearners, "the reduce + Adam launch is k_train_sweep_adam: its table carries the learners");

extern "C" int susnet_spatial_train_sweep_table_bytes(int32_t n_learners, uint64_t *bytes_out) {
    if (int rc = check_n_learners("susnet_spatial_train_sweep_table_bytes", n_learners, SUSNET_SPATIAL_SWEEP_MAX_LEARNERS)) return rc;
    if (!bytes_out) return fail(SUSNET_E_INVALID, "susnet_spatial_train_sweep_table_bytes: null bytes_out");
    *bytes_out = sp_sweep_table_bytes(n_learners);
    return SUSNET_OK;
}

// the first field of what shapes the step in which learner k's io differs from learner 0's, or an empty string
static std::string sp_sweep_mismatch(const susnet_env *e0, const susnet_spatial_train_io &i0, const SpTrainChecked &c0, const susnet_env *e,
                                     const susnet_spatial_train_io &io, const SpTrainChecked &c, bool drops) {
    const auto S = [](int v) { return std::to_string(v); };
    if (e->c.A != e0->c.A || e->c.n_imp != e0->c.n_imp) return "agent count";
    if (io.n != i0.n) return "n";
    for (int tm = 0; tm < 2; tm++)
        if ((io.team[tm].enabled != 0) != (i0.team[tm].enabled != 0)) return "team[" + S(tm) + "].enabled";
    for (int tm = 0; tm < 2; tm++) {
        if (!i0.team[tm].enabled) continue;
        const susnet_spatial_net &a = i0.net[tm], &b = io.net[tm];
        const std::string net = "net[" + S(tm) + "].", team = "team[" + S(tm) + "].";
        const std::pair<const char *, bool> scalars[] = {{"T", a.T != b.T}, {"N", a.N != b.N}, {"C", a.C != b.C}, {"Fn", a.Fn != b.Fn},
                                                         {"n_conv", a.n_conv != b.n_conv}, {"k", a.k != b.k}};
        for (const auto &f : scalars)
            if (f.second) return net + f.first;
        for (int l = 0; l < a.n_conv; l++) {
            const std::string at = "[" + S(l) + "]";
            if (a.conv_out[l] != b.conv_out[l]) return net + "conv_out" + at;
            if (a.conv_stride[l] != b.conv_stride[l]) return net + "conv_stride" + at;
            if (a.conv_padding[l] != b.conv_padding[l]) return net + "conv_padding" + at;
            if (a.conv_dilation[l] != b.conv_dilation[l]) return net + "conv_dilation" + at;
        }
        if (a.rnn_layers != b.rnn_layers) return net + "rnn_layers";
        if (a.rnn_hidden != b.rnn_hidden) return net + "rnn_hidden";
        if (io.team[tm].n_dims != i0.team[tm].n_dims) return team + "n_dims";
        if (memcmp(io.team[tm].dims, i0.team[tm].dims, sizeof(int32_t) * (size_t)i0.team[tm].n_dims) != 0) return team + "dims";
    }
    for (int d = 0; d < 3; d++)
        if (io.spatial_stride[d] != i0.spatial_stride[d]) return "spatial_stride[" + S(d) + "]";
    for (int d = 0; d < 3 && c0.Fn > 0; d++)
        if (io.non_spatial_stride[d] != i0.non_spatial_stride[d]) return "non_spatial_stride[" + S(d) + "]";
    for (int tm = 0; tm < 2 && drops; tm++)
        if (c.masked[tm] != c0.masked[tm]) return "drops: whether team[" + S(tm) + "] is masked (a p > 0 with more than one RNN layer)";
    return "";
}

extern "C" int susnet_spatial_train_sweep(susnet_env *const *envs, const susnet_spatial_train_io *ios, const susnet_rnn_dropout *drops, int32_t n_learners,
                                          void *table, uint64_t table_bytes, void *stream) {
    const std::string entry = "susnet_spatial_train_sweep: ";
    if (!envs || !ios) return fail(SUSNET_E_INVALID, entry + "null envs / ios");
    if (int rc = check_n_learners("susnet_spatial_train_sweep", n_learners, SUSNET_SPATIAL_SWEEP_MAX_LEARNERS)) return rc;
    const int K = n_learners;
    const auto who = [](int k, const std::string &what) { return sweep_learner("susnet_spatial_train_sweep", k, what); };
    std::vector<SpTrainChecked> cs((size_t)K);
    for (int k = 0; k < K; k++) { // each learner passes its own call's checks ...
        if (!envs[k]) return fail(SUSNET_E_INVALID, who(k, "null handle"));
        if (int rc = sp_train_check(envs[k], &ios[k], drops ? drops + 2 * k : nullptr, drops ? "susnet_spatial_train_step_dropout" : "susnet_spatial_train_step",
                                    cs[(size_t)k]))
            return fail(rc, who(k, g_err));
    }
    for (int k = 1; k < K; k++) { // ... and all agree on what shapes the step
        const std::string field = sp_sweep_mismatch(envs[0], ios[0], cs[0], envs[k], ios[k], cs[(size_t)k], drops != nullptr);
        if (!field.empty()) return fail(SUSNET_E_INVALID, who(k, field + " differs from learner 0's (a sweep runs learners of one shape)"));
        if (cs[(size_t)k].pl.bytes != cs[0].pl.bytes || cs[(size_t)k].pl.G != cs[0].pl.G || cs[(size_t)k].pl.Gconv != cs[0].pl.Gconv)
            return fail(SUSNET_E_INVALID, who(k, "workspace plan differs from learner 0's"));
    }
    if (int rc = check_learners_apart("susnet_spatial_train_sweep", ios, K)) return rc;
    const uint64_t need = sp_sweep_table_bytes(K);
    if (!table || table_bytes < need || (reinterpret_cast<uintptr_t>(table) & 255u))
        return fail(SUSNET_E_INVALID, entry + "table missing, smaller than susnet_spatial_train_sweep_table_bytes (" + std::to_string((unsigned long long)need) +
                                          " bytes) or not 256-byte aligned");
    // what the learners share, and each one's own
    const SpTrainPlan &pl = cs[0].pl;
    const susnet_spatial_train_io &i0 = ios[0];
    SpSweepShared sh{};
    sh.net[0] = pl.net[0], sh.net[1] = pl.net[1];
    for (int d = 0; d < 3; d++) sh.sp_stride[d] = i0.spatial_stride[d], sh.ns_stride[d] = cs[0].Fn > 0 ? i0.non_spatial_stride[d] : 0;
    sh.n = i0.n, sh.A = (int32_t)envs[0]->c.A, sh.n_imp = (int32_t)envs[0]->c.n_imp;
    sh.off_lists = pl.off_lists, sh.off_counts = pl.off_counts, sh.off_gacc[0] = pl.off_gacc[0], sh.off_gacc[1] = pl.off_gacc[1], sh.off_partial = pl.off_partial;
    sh.off_X = pl.off_X, sh.off_Xt = pl.off_Xt, sh.off_act = pl.off_act, sh.off_dact = pl.off_dact, sh.off_dX = pl.off_dX, sh.off_tact = pl.off_tact;
    sh.off_hs = pl.off_hs, sh.off_ds = pl.off_ds, sh.off_zs = pl.off_zs, sh.off_ms = pl.off_ms;
    SpSweepLearner learners[kSpSweepMaxLearners] = {};
    TrainTable tab[2] = {};
    TrainNet anet[2] = {};
    for (int tm = 0; tm < 2; tm++) anet[tm].P = pl.net[tm].P, anet[tm].Pp = pl.net[tm].Pp;
    for (int k = 0; k < K; k++) {
        const susnet_spatial_train_io &io = ios[k];
        const TrBuffers b = tr_buffers(io.workspace, pl);
        SpSweepLearner &l = learners[k];
        l.spatial = io.spatial, l.next_spatial = io.next_spatial, l.non_spatial = io.non_spatial, l.next_non_spatial = io.next_non_spatial;
        l.actions = io.actions, l.rewards = io.rewards, l.dones = io.dones, l.imposters = io.imposters, l.idx = io.indices;
        l.max_size = io.max_size, l.workspace = static_cast<char *>(io.workspace), l.losses = io.losses_out, l.gamma = (float)io.gamma;
        for (int tm = 0; tm < 2; tm++) {
            const susnet_dqn_team &T = io.team[tm];
            if (!T.enabled) continue;
            l.prm[tm] = T.params, l.tgt[tm] = T.target_params, l.step[tm] = T.step;
            const SpDrop &d = cs[(size_t)k].dr[tm];
            l.dr[tm] = SpDropArgs{d.k0, d.k1, d.off_lo, d.off_hi, {d.thr[0], d.thr[1]}, {d.scale[0], d.scale[1]}, d.row_base};
            tab[tm].l[k] = TrainLearner{TrainRing{}, T.params, T.target_params, T.exp_avg, T.exp_avg_sq, T.step, b.lists, b.counts, b.gacc[tm], b.partial,
                                        io.losses_out, nullptr, T.lr, T.beta1, T.beta2, T.eps, (float)io.gamma, 0};
        }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    SpSweepTable *dtab = static_cast<SpSweepTable *>(table);
    HIP_TRY(sp_train_sweep_select_launch(sh, learners, K, dtab, st));
    if (i0.n == 0) return SUSNET_OK;
    const unsigned Ku = (unsigned)K;
    for (int agent = 0; agent < envs[0]->c.A; agent++)
        for (int tm = 0; tm < 2; tm++) { // imposter team, then crew team (train.py:91-99)
            if (!i0.team[tm].enabled) continue;
            HIP_TRY(sp_train_sweep_update_launch(dtab, K, agent, tm, (int)pl.G, (int)pl.Gconv, cs[0].masked[tm], st));
            hipLaunchKernelGGL(k_train_sweep_adam, dim3((unsigned)((pl.net[tm].P + 1 + 255) / 256), Ku), dim3(256), 0, st, tab[tm], anet[tm], agent, tm, (int)pl.G);
            HIP_TRY(hipGetLastError());
        }
    return SUSNET_OK;
}
