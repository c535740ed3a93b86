// the SpatialDQN learner's kernels (susnet_spatial_train.h: susnet_spatial_train_step) -- a translation unit of its own
#include "susnet_spatial_train.h"

#include "susnet_dropout.h"
#include "susnet_host.h" // lds_opt_in
#include "susnet_spatial.h" // sp_tanh: the forward's tanh
#include "susnet_train_core.h"

namespace susnet {

// LDS of k_sp_train_rnn (floats): the dense learner's plan -- two activation and two dZ buffers of kMtMaxHidden units, transposed
// [unit][sample] with row stride kTrSP -- for the head; the recurrence itself lives in the workgroup's workspace slices
constexpr int kStBuf = kMtMaxHidden * kTrSP;
constexpr int kStOH0 = 0, kStOH1 = kStBuf, kStODA = 2 * kStBuf, kStODB = 3 * kStBuf, kStOY = 4 * kStBuf, kStOAct = kStOY + kTrTS,
              kStOPos = kStOAct + kTrTS, kStORow = kStOPos + kTrTS, kStORed = kStORow + kTrTS, kStLdsFloats = kStORed + kTrThreads;
constexpr int kStLdsBytes = kStLdsFloats * 4;
static_assert(kStLdsBytes <= 160 * 1024, "gfx950 LDS");
static_assert(kTrThreads >= kMtMaxHidden, "a thread per unit for the bias gradients");

__device__ __forceinline__ int64_t st_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ---- k_sp_train_select: ONE workgroup of kTrThreads; tr_select with batch positions in the lists ----
// -- and the two teams' network descriptions go from the kernel arguments to the workspace, where the update's kernels read them: their
// loops over layers index the description, and an indexed kernel argument would be copied to private memory first
__global__ __launch_bounds__(kTrThreads) void k_sp_train_select(SpTrainBatch b, SpTrainNet net0, SpTrainNet net1, SpTrainNet *nets, int32_t *lists,
                                                                int32_t *counts, float *gacc0, float *gacc1, float *losses) {
    extern __shared__ int32_t st_scan[];
    if (threadIdx.x == 0) {
        nets[0] = net0;
        nets[1] = net1;
    }
    tr_select<true>(b, b.idx, b.n, lists, counts, gacc0, net0.P, gacc1, net1.P, losses, st_scan);
}

// ---- k_sp_train_conv: the convolutions of one update's rows, online network on the states and target network on the next states ----
__global__ __launch_bounds__(kStConvThreads) void k_sp_train_conv(SpTrainBatch b, const SpTrainNet *__restrict__ netp, SpTrainWs ws, const float *__restrict__ prm,
                                                                  const float *__restrict__ tgt, const int32_t *__restrict__ lists,
                                                                  const int32_t *__restrict__ counts, int agent, int team) {
#include "susnet_spatial_train_conv_body.h"
}

// one step of the recurrence on a tile: h[l][t] = tanh(b_ih + b_hh + W_ih in + W_hh h[l][t-1]), in = the RNN input rows X (l = 0; a column
// past nvalid is a zero operand) or h[l-1][t].  hs: the workgroup's slice, [l][t][unit][32]
// DROP: in = m[l-1][t] h[l-1][t], the multipliers read from ms ([l][t][unit][32], l < L - 1), and the step writes its own m[l][t] there
// (susnet_dropout.h: net `dnet`, the row = the batch position list[j0 + s])
template <bool DROP>
__device__ __forceinline__ void st_rnn_step(const SpTrainNet &net, const float *__restrict__ P, int l, int t, const float *X, int64_t j0, int nvalid,
                                            float *hs, int wave, int lane, const SpDrop *dr, int dnet, const int32_t *list, int64_t bn, float *ms) {
    const int H = net.H, R = net.R, T = net.T, s = lane & 31;
    const bool svalid = s < nvalid;
    const float *Wih = P + net.oWih[l], *Whh = P + net.oWhh[l], *bih = P + net.oBih[l], *bhh = P + net.oBhh[l];
    const float *xrow = X + ((size_t)(j0 + (svalid ? s : 0)) * T + t) * R;
    const float *hin = hs + ((size_t)((l > 0 ? l - 1 : 0) * T + t) * H) * kTrTS;
    const float *hprev = hs + ((size_t)(l * T + (t > 0 ? t - 1 : 0)) * H) * kTrTS;
    float *hout = hs + ((size_t)(l * T + t) * H) * kTrTS;
    [[maybe_unused]] const float *msin = nullptr;
    [[maybe_unused]] float *mout = nullptr;
    if constexpr (DROP) {
        msin = ms + ((size_t)((l > 0 ? l - 1 : 0) * T + t) * H) * kTrTS;
        mout = ms + ((size_t)(l * T + t) * H) * kTrTS;
    }
    const int nt_count = (H + 31) / 32;
    for (int nt = wave; nt < nt_count; nt += kTrWaves) {
        const int n0 = nt * 32;
        tr_f32x16 acc = {};
        if (l == 0)
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Wih[(size_t)(n0 + i) * R + p] : 0.0f; },
                          [&](int p, int j) { return svalid ? xrow[p] : 0.0f; }, R, acc, lane);
        else if constexpr (DROP)
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Wih[(size_t)(n0 + i) * H + p] : 0.0f; },
                          [&](int p, int j) { return msin[p * kTrTS + j] * hin[p * kTrTS + j]; }, H, acc, lane);
        else
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Wih[(size_t)(n0 + i) * H + p] : 0.0f; },
                          [&](int p, int j) { return hin[p * kTrTS + j]; }, H, acc, lane);
        if (t > 0)
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Whh[(size_t)(n0 + i) * H + p] : 0.0f; },
                          [&](int p, int j) { return hprev[p * kTrTS + j]; }, H, acc, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int n = n0 + tr_row(r, lane);
            if (n < H) hout[n * kTrTS + s] = sp_tanh(acc[r] + (bih[n] + bhh[n]));
        }
        if constexpr (DROP) {
            if (l < net.L - 1) {
                const int64_t row = st_clamp(svalid ? list[j0 + s] : 0, bn);
#pragma unroll
                for (int q = 0; q < 4; q++) { // registers 4 q .. 4 q + 3: four consecutive units, one Philox block
                    float m[4];
                    sp_drop4(*dr, dnet, row, t, l, (n0 + tr_row(4 * q, lane)) >> 2, m);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int n = n0 + tr_row(4 * q + j, lane);
                        if (n < H) mout[n * kTrTS + s] = m[j];
                    }
                }
            }
        }
    }
}

// the whole network behind the convolutions on one tile: recurrence into hs, then the head on LDS (layer l writes buffer l & 1; layer 0
// reads the top layer's last hidden state, copied into buffer 1).  SAVE: the head's hidden pre-activations also go to zsave, as
// inst_mlp_train.hip's mt_forward keeps them
template <bool SAVE, bool DROP>
__device__ __forceinline__ void st_forward(const SpTrainNet &net, const float *__restrict__ P, const float *X, int64_t j0, int nvalid, float *hs,
                                           float *lds, float *zsave, int tid, int wave, int lane, const SpDrop *dr, int dnet, const int32_t *list,
                                           int64_t bn, float *ms) {
    for (int t = 0; t < net.T; t++)
        for (int l = 0; l < net.L; l++) {
            st_rnn_step<DROP>(net, P, l, t, X, j0, nvalid, hs, wave, lane, dr, dnet, list, bn, ms);
            __syncthreads();
        }
    const float *htop = hs + ((size_t)((net.L - 1) * net.T + net.T - 1) * net.H) * kTrTS;
    for (int e = tid; e < net.H * kTrTS; e += kTrThreads) lds[kStOH1 + (e >> 5) * kTrSP + (e & 31)] = htop[e];
    __syncthreads();
    const MlpTrainNet &hd = net.head;
    for (int l = 0; l < hd.nl; l++) {
        float *zout = lds + ((l & 1) ? kStOH1 : kStOH0);
        const float *zin = lds + ((l & 1) ? kStOH0 : kStOH1);
        tr_forward_layer(P + hd.oW[l], P + hd.oB[l], hd.d[l], hd.d[l + 1], zin, l > 0 ? P[hd.oA[l - 1]] : 1.0f, l == 0, zout, wave, lane);
        __syncthreads();
        if (SAVE && l < hd.nl - 1) {
            float *dst = zsave + hd.zo[l];
            for (int e = tid; e < hd.d[l + 1] * kTrTS; e += kTrThreads) dst[e] = zout[(e >> 5) * kTrSP + (e & 31)];
        }
    }
}

// ---- k_sp_train_rnn: one (agent, team) update's gradient partials behind the convolutions; workgroup blockIdx.x of gridDim.x ----
__global__ __launch_bounds__(kTrThreads) void k_sp_train_rnn(SpTrainBatch b, const SpTrainNet *__restrict__ netp, SpTrainWs ws, const float *__restrict__ prm,
                                                             const float *__restrict__ tgt, const int32_t *__restrict__ lists,
                                                             const int32_t *__restrict__ counts, int agent, int team, float gamma,
                                                             float *__restrict__ partial, float *step) {
#define SP_TRAIN_DROPOUT 0
#include "susnet_spatial_train_rnn_body.h"
#undef SP_TRAIN_DROPOUT
}
// the dropout form (susnet_spatial_train_step_dropout): dr.agent == agent; ms: [G][(L - 1) T H 32] floats
__global__ __launch_bounds__(kTrThreads) void k_sp_train_rnn_dropout(SpTrainBatch b, const SpTrainNet *__restrict__ netp, SpTrainWs ws,
                                                                     const float *__restrict__ prm, const float *__restrict__ tgt,
                                                                     const int32_t *__restrict__ lists, const int32_t *__restrict__ counts, int agent,
                                                                     int team, float gamma, float *__restrict__ partial, float *step, SpDrop dr,
                                                                     float *ms) {
#define SP_TRAIN_DROPOUT 1
#include "susnet_spatial_train_rnn_body.h"
#undef SP_TRAIN_DROPOUT
}

// ---- k_sp_train_conv_bwd: the convolutions' backward of one update; workgroup blockIdx.x of gridDim.x owns images blockIdx.x + i gridDim.x ----
__global__ __launch_bounds__(kStConvThreads) void k_sp_train_conv_bwd(SpTrainBatch b, const SpTrainNet *__restrict__ netp, SpTrainWs ws, const float *__restrict__ prm,
                                                                      const int32_t *__restrict__ lists, const int32_t *__restrict__ counts, int agent,
                                                                      int team, float *__restrict__ partial) {
#include "susnet_spatial_train_conv_bwd_body.h"
}

// ---- the sweep forms (susnet_spatial_train.h): learner blockIdx.y of the table; every body is the single learner's text ----
// what the bodies name as kernel arguments, from the shared record and the learner's own
__device__ __forceinline__ SpTrainBatch st_sweep_batch(const SpSweepShared &sh, const SpSweepLearner &lrn) {
    SpTrainBatch b;
    b.spatial = lrn.spatial, b.next_spatial = lrn.next_spatial, b.non_spatial = lrn.non_spatial, b.next_non_spatial = lrn.next_non_spatial;
#pragma unroll
    for (int d = 0; d < 3; d++) b.sp_stride[d] = sh.sp_stride[d], b.ns_stride[d] = sh.ns_stride[d];
    b.actions = lrn.actions, b.rewards = lrn.rewards, b.dones = lrn.dones, b.imposters = lrn.imposters, b.idx = lrn.idx;
    b.max_size = lrn.max_size, b.n = sh.n, b.A = sh.A, b.n_imp = sh.n_imp;
    return b;
}
__device__ __forceinline__ SpTrainWs st_sweep_ws(const SpSweepShared &sh, const SpSweepLearner &lrn) {
    const auto at = [&](uint64_t off) { return reinterpret_cast<float *>(lrn.workspace + off); };
    return SpTrainWs{at(sh.off_X), at(sh.off_Xt), at(sh.off_act), at(sh.off_dact), at(sh.off_dX), at(sh.off_tact), at(sh.off_hs), at(sh.off_ds), at(sh.off_zs)};
}
// `first`: the table index of a.l[0]; the launch with first == 0 also writes the shared record.  A workgroup reads its learner from the
// ARGUMENTS (nothing another workgroup of this launch writes), the later launches read the table
__global__ __launch_bounds__(kTrThreads) void k_sp_train_sweep_select(SpSweepShared sh, SpSweepSelArgs a, int first, SpSweepTable *table) {
    extern __shared__ int32_t st_scan[];
    const SpSweepLearner &lrn = a.l[blockIdx.y];
    if (threadIdx.x == 0) {
        if (first == 0 && blockIdx.y == 0) table->sh = sh;
        table->l[first + blockIdx.y] = lrn;
    }
    const SpTrainBatch b = st_sweep_batch(sh, lrn);
    tr_select<true>(b, b.idx, b.n, reinterpret_cast<int32_t *>(lrn.workspace + sh.off_lists), reinterpret_cast<int32_t *>(lrn.workspace + sh.off_counts),
                    reinterpret_cast<float *>(lrn.workspace + sh.off_gacc[0]), sh.net[0].P, reinterpret_cast<float *>(lrn.workspace + sh.off_gacc[1]),
                    sh.net[1].P, lrn.losses, st_scan);
}
// the arguments of the single learner's kernels, as locals of the same names
#define SP_SWEEP_ARGS                                                                                                        \
    const SpSweepShared &sh = table->sh;                                                                                     \
    const SpSweepLearner &lrn = table->l[blockIdx.y];                                                                        \
    const SpTrainBatch b = st_sweep_batch(sh, lrn);                                                                          \
    const SpTrainNet *__restrict__ netp = &sh.net[team];                                                                     \
    const SpTrainWs ws = st_sweep_ws(sh, lrn);                                                                               \
    const float *__restrict__ prm = lrn.prm[team];                                                                           \
    [[maybe_unused]] const float *__restrict__ tgt = lrn.tgt[team];                                                          \
    const int32_t *__restrict__ lists = reinterpret_cast<const int32_t *>(lrn.workspace + sh.off_lists);                     \
    const int32_t *__restrict__ counts = reinterpret_cast<const int32_t *>(lrn.workspace + sh.off_counts);                   \
    [[maybe_unused]] float *__restrict__ partial = reinterpret_cast<float *>(lrn.workspace + sh.off_partial);
#define SP_SWEEP_RNN_ARGS                                                                                                    \
    SP_SWEEP_ARGS                                                                                                            \
    const float gamma = lrn.gamma;                                                                                           \
    float *step = lrn.step[team];

__global__ __launch_bounds__(kStConvThreads) void k_sp_train_sweep_conv(const SpSweepTable *__restrict__ table, int agent, int team) {
    SP_SWEEP_ARGS
#include "susnet_spatial_train_conv_body.h"
}
__global__ __launch_bounds__(kTrThreads) void k_sp_train_sweep_rnn(const SpSweepTable *__restrict__ table, int agent, int team) {
    SP_SWEEP_RNN_ARGS
#define SP_TRAIN_DROPOUT 0
#include "susnet_spatial_train_rnn_body.h"
#undef SP_TRAIN_DROPOUT
}
__global__ __launch_bounds__(kTrThreads) void k_sp_train_sweep_rnn_dropout(const SpSweepTable *__restrict__ table, int agent, int team) {
    SP_SWEEP_RNN_ARGS
    const SpDropArgs &da = lrn.dr[team];
    const SpDrop dr{da.k0, da.k1, da.off_lo, da.off_hi, {da.thr[0], da.thr[1]}, {da.scale[0], da.scale[1]}, da.row_base, agent};
    float *ms = reinterpret_cast<float *>(lrn.workspace + sh.off_ms);
#define SP_TRAIN_DROPOUT 1
#include "susnet_spatial_train_rnn_body.h"
#undef SP_TRAIN_DROPOUT
}
__global__ __launch_bounds__(kStConvThreads) void k_sp_train_sweep_conv_bwd(const SpSweepTable *__restrict__ table, int agent, int team) {
    SP_SWEEP_ARGS
#include "susnet_spatial_train_conv_bwd_body.h"
}
#undef SP_SWEEP_RNN_ARGS
#undef SP_SWEEP_ARGS

hipError_t sp_train_sweep_select_launch(const SpSweepShared &sh, const SpSweepLearner *l, int K, SpSweepTable *table, hipStream_t st) {
    for (int first = 0; first < K; first += kSpSweepSelLearners) {
        const int count = K - first < kSpSweepSelLearners ? K - first : kSpSweepSelLearners;
        SpSweepSelArgs a{};
        for (int k = 0; k < count; k++) a.l[k] = l[first + k];
        hipLaunchKernelGGL(k_sp_train_sweep_select, dim3(1, (unsigned)count), dim3(kTrThreads), kTrThreads * 4, st, sh, a, first, table);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t sp_train_sweep_update_launch(const SpSweepTable *table, int K, int agent, int team, int G, int Gconv, bool dropout, hipStream_t st) {
    // the recurrence kernels' dynamic-LDS ceilings, as sp_train_update_launch sets its kernels'
    static LdsOptIn opted, opted_drop;
    if (hipError_t e = dropout ? lds_opt_in(reinterpret_cast<const void *>(&k_sp_train_sweep_rnn_dropout), kStLdsBytes, opted_drop)
                               : lds_opt_in(reinterpret_cast<const void *>(&k_sp_train_sweep_rnn), kStLdsBytes, opted))
        return e;
    const unsigned Ku = (unsigned)K;
    hipLaunchKernelGGL(k_sp_train_sweep_conv, dim3((unsigned)Gconv, Ku), dim3(kStConvThreads), 0, st, table, agent, team);
    if (hipError_t e = hipGetLastError()) return e;
    if (dropout) hipLaunchKernelGGL(k_sp_train_sweep_rnn_dropout, dim3((unsigned)G, Ku), dim3(kTrThreads), kStLdsBytes, st, table, agent, team);
    else hipLaunchKernelGGL(k_sp_train_sweep_rnn, dim3((unsigned)G, Ku), dim3(kTrThreads), kStLdsBytes, st, table, agent, team);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_sp_train_sweep_conv_bwd, dim3((unsigned)G, Ku), dim3(kStConvThreads), 0, st, table, agent, team);
    return hipGetLastError();
}

hipError_t sp_train_select_launch(const SpTrainBatch &b, const SpTrainNet &net0, const SpTrainNet &net1, SpTrainNet *nets, int32_t *lists,
                                  int32_t *counts, float *gacc0, float *gacc1, float *losses, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_train_select, dim3(1), dim3(kTrThreads), kTrThreads * 4, st, b, net0, net1, nets, lists, counts, gacc0, gacc1, losses);
    return hipGetLastError();
}

hipError_t sp_train_update_launch(const SpTrainBatch &b, const SpTrainNet *net, const SpTrainWs &ws, const float *prm, const float *tgt,
                                  const int32_t *lists, const int32_t *counts, int agent, int team, float gamma, float *partial, float *step, int G,
                                  int Gconv, hipStream_t st, const SpDrop *dr, float *ms) {
    // the recurrence kernel's dynamic-LDS ceiling, set once per device (not repeated inside a capture after the first eager step)
    static LdsOptIn opted, opted_drop;
    if (hipError_t e = dr ? lds_opt_in(reinterpret_cast<const void *>(&k_sp_train_rnn_dropout), kStLdsBytes, opted_drop)
                          : lds_opt_in(reinterpret_cast<const void *>(&k_sp_train_rnn), kStLdsBytes, opted))
        return e;
    hipLaunchKernelGGL(k_sp_train_conv, dim3((unsigned)Gconv), dim3(kStConvThreads), 0, st, b, net, ws, prm, tgt, lists, counts, agent, team);
    if (hipError_t e = hipGetLastError()) return e;
    if (dr) { // (the update's agent goes into the mask's counter)
        SpDrop d = *dr;
        d.agent = agent;
        hipLaunchKernelGGL(k_sp_train_rnn_dropout, dim3((unsigned)G), dim3(kTrThreads), kStLdsBytes, st, b, net, ws, prm, tgt, lists, counts, agent,
                           team, gamma, partial, step, d, ms);
    } else
        hipLaunchKernelGGL(k_sp_train_rnn, dim3((unsigned)G), dim3(kTrThreads), kStLdsBytes, st, b, net, ws, prm, tgt, lists, counts, agent, team,
                           gamma, partial, step);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_sp_train_conv_bwd, dim3((unsigned)G), dim3(kStConvThreads), 0, st, b, net, ws, prm, lists, counts, agent, team, partial);
    return hipGetLastError();
}

} // namespace susnet
