// the dense learner's kernels (susnet_mlp_train.h: susnet_mlp_train_step) -- a translation unit of its own
#include "susnet_mlp_train.h"

#include "susnet_host.h" // lds_opt_in
#include "susnet_train_core.h"

namespace susnet {

// LDS (floats): two activation buffers and two dZ buffers of kMtMaxHidden units, transposed [unit][sample] with row stride kTrSP
constexpr int kMtBuf = kMtMaxHidden * kTrSP;
constexpr int kMtOH0 = 0, kMtOH1 = kMtBuf, kMtODA = 2 * kMtBuf, kMtODB = 3 * kMtBuf, kMtOY = 4 * kMtBuf, kMtOAct = kMtOY + kTrTS,
              kMtOPos = kMtOAct + kTrTS, kMtORow = kMtOPos + kTrTS, kMtLdsFloats = kMtORow + kTrTS;
constexpr int kMtLdsBytes = kMtLdsFloats * 4;
static_assert(kMtLdsBytes <= 160 * 1024, "gfx950 LDS");
static_assert(kMtMaxOut <= kMtMaxHidden && kTrThreads >= kMtMaxHidden, "a thread per unit for the bias gradients");

// ---- k_mlp_train_select: ONE workgroup of kTrThreads; tr_select with batch positions in the lists ----
__global__ __launch_bounds__(kTrThreads) void k_mlp_train_select(MlpTrainBatch b, int32_t *lists, int32_t *counts, float *gacc0, int P0, float *gacc1,
                                                                 int P1, float *losses) {
    extern __shared__ int32_t mt_scan[];
    tr_select<true>(b, b.idx, b.n, lists, counts, gacc0, P0, gacc1, P1, losses, mt_scan);
}

// layer 1 from the feature rows in global memory: Z[n][s] = b[n] + sum_k W[n][k] X[pos[s]][k]; a column past nvalid is a zero operand
__device__ __forceinline__ void mt_forward_input(const float *__restrict__ W, const float *__restrict__ bias, int dk, int dn, const float *__restrict__ X,
                                                 const int32_t *pos, int nvalid, float *zout, int wave, int lane) {
    const int nt_count = (dn + 31) / 32;
    const bool svalid = (lane & 31) < nvalid;
    const float *xrow = X + (size_t)pos[lane & 31] * dk;
    for (int nt = wave; nt < nt_count; nt += kTrWaves) {
        const int n0 = nt * 32;
        tr_f32x16 acc = {};
        acc = tr_mfma([&](int i, int p) { return n0 + i < dn ? W[(size_t)(n0 + i) * dk + p] : 0.0f; }, [&](int p, int j) { return svalid ? xrow[p] : 0.0f; },
                      dk, acc, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int n = n0 + tr_row(r, lane);
            if (n < dn) zout[n * kTrSP + (lane & 31)] = acc[r] + bias[n];
        }
    }
}

// the whole stack on one tile; layer l writes buffer l & 1.  SAVE: the hidden pre-activations also go to the workgroup's slice, element e of
// layer l's [unit][32] block by thread e % kTrThreads (the backward pass reads it back with the same thread)
template <bool SAVE>
__device__ __forceinline__ void mt_forward(const MlpTrainNet &net, const float *__restrict__ prm, const float *__restrict__ X, const int32_t *pos,
                                           int nvalid, float *lds, float *zsave, int t, int wave, int lane) {
#pragma unroll
    for (int l = 0; l < kMtMaxLayers; l++) {
        if (l < net.nl) {
            float *zout = lds + ((l & 1) ? kMtOH1 : kMtOH0);
            const float *zin = lds + ((l & 1) ? kMtOH0 : kMtOH1);
            if (l == 0) mt_forward_input(prm + net.oW[0], prm + net.oB[0], net.d[0], net.d[1], X, pos, nvalid, zout, wave, lane);
            else tr_forward_layer(prm + net.oW[l], prm + net.oB[l], net.d[l], net.d[l + 1], zin, prm[net.oA[l > 0 ? l - 1 : 0]], false, zout, wave, lane);
            __syncthreads();
            if (SAVE && l < net.nl - 1) {
                float *dst = zsave + net.zo[l < 6 ? l : 5];
                for (int e = t; e < net.d[l + 1] * kTrTS; e += kTrThreads) dst[e] = zout[(e >> 5) * kTrSP + (e & 31)];
            }
        }
    }
}

// ---- k_mlp_train_grad: one (agent, team) update's gradient partials; workgroup blockIdx.x of gridDim.x ----
__global__ __launch_bounds__(kTrThreads) void k_mlp_train_grad(MlpTrainBatch b, MlpTrainNet net, const float *__restrict__ prm, const float *__restrict__ tgt,
                                                               const int32_t *__restrict__ lists, const int32_t *__restrict__ counts, int agent, int team,
                                                               float gamma, float *__restrict__ partial, float *__restrict__ zsave_all, float *step) {
#include "susnet_mlp_train_grad_body.h"
}

// ---- the sweep forms (susnet_mlp_train.h): learner blockIdx.y of the table; the bodies are the single learner's ----
__global__ __launch_bounds__(kTrThreads) void k_mlp_train_sweep_select(MlpSweepSelTable tab, int64_t n, int A, int n_imp, int P0, int P1) {
    extern __shared__ int32_t mt_scan[];
    const MlpSweepSelLearner &a = tab.l[blockIdx.y];
    MlpTrainBatch b{}; // (tr_select reads imposters, n_imp, max_size and A of it)
    b.imposters = a.imposters, b.max_size = a.max_size, b.A = A, b.n_imp = n_imp;
    tr_select<true>(b, a.idx, n, a.lists, a.counts, a.gacc0, P0, a.gacc1, P1, a.losses, mt_scan);
}
__global__ __launch_bounds__(kTrThreads) void k_mlp_train_sweep_grad(MlpSweepTable tab, MlpTrainNet net, int64_t n, int A, int n_imp, int agent, int team) {
    // the arguments of k_mlp_train_grad, as locals of the same names
    const MlpSweepLearner &lrn = tab.l[blockIdx.y];
    const MlpTrainBatch b{lrn.feat, lrn.next_feat, lrn.actions, lrn.rewards, lrn.dones, lrn.imposters, lrn.idx, lrn.max_size, n, A, n_imp};
    const float *__restrict__ prm = lrn.prm;
    const float *__restrict__ tgt = lrn.tgt;
    const int32_t *__restrict__ lists = lrn.lists;
    const int32_t *__restrict__ counts = lrn.counts;
    const float gamma = lrn.gamma;
    float *__restrict__ partial = lrn.partial;
    float *__restrict__ zsave_all = lrn.zsave;
    float *step = lrn.step;
#include "susnet_mlp_train_grad_body.h"
}

hipError_t mlp_train_select_launch(const MlpTrainBatch &b, int32_t *lists, int32_t *counts, float *gacc0, int P0, float *gacc1, int P1, float *losses,
                                   hipStream_t st) {
    hipLaunchKernelGGL(k_mlp_train_select, dim3(1), dim3(kTrThreads), kTrThreads * 4, st, b, lists, counts, gacc0, P0, gacc1, P1, losses);
    return hipGetLastError();
}

hipError_t mlp_train_grad_launch(const MlpTrainBatch &b, const MlpTrainNet &net, const float *prm, const float *tgt, const int32_t *lists,
                                 const int32_t *counts, int agent, int team, float gamma, float *partial, float *zsave, float *step, int G, hipStream_t st) {
    // the kernel's dynamic-LDS ceiling, set once per device (not repeated inside a capture after the first eager step)
    static LdsOptIn opted;
    if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_mlp_train_grad), kMtLdsBytes, opted)) return e;
    hipLaunchKernelGGL(k_mlp_train_grad, dim3((unsigned)G), dim3(kTrThreads), kMtLdsBytes, st, b, net, prm, tgt, lists, counts, agent, team, gamma, partial,
                       zsave, step);
    return hipGetLastError();
}

hipError_t mlp_train_sweep_select_launch(const MlpSweepSelTable &tab, int K, int64_t n, int A, int n_imp, int P0, int P1, hipStream_t st) {
    hipLaunchKernelGGL(k_mlp_train_sweep_select, dim3(1, (unsigned)K), dim3(kTrThreads), kTrThreads * 4, st, tab, n, A, n_imp, P0, P1);
    return hipGetLastError();
}

hipError_t mlp_train_sweep_grad_launch(const MlpSweepTable &tab, int K, const MlpTrainNet &net, int64_t n, int A, int n_imp, int agent, int team, int G,
                                       hipStream_t st) {
    static LdsOptIn opted; // (as mlp_train_grad_launch)
    if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_mlp_train_sweep_grad), kMtLdsBytes, opted)) return e;
    hipLaunchKernelGGL(k_mlp_train_sweep_grad, dim3((unsigned)G, (unsigned)K), dim3(kTrThreads), kMtLdsBytes, st, tab, net, n, A, n_imp, agent, team);
    return hipGetLastError();
}

} // namespace susnet
