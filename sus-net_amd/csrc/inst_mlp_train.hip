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
    extern __shared__ float lds[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int count = counts[2 * agent + team];
    if (count == 0) return; // an empty team takes no step (train.py:101): k_train_adam does nothing either
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    if (blockIdx.x == 0 && t == 0) step[0] += 1.0f; // (k_train_adam reads it after this launch)
    const int nl = net.nl, n_out = net.d[nl], F = net.d[0];
    float *out = partial + (size_t)blockIdx.x * net.Pp;
    float *zsave = zsave_all + (size_t)blockIdx.x * net.Z;
    float lacc = 0.0f, sacc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float inv_n = 2.0f / (float)count; // mse_loss backward: 2 (x - y) / numel
    int32_t *pos = reinterpret_cast<int32_t *>(lds + kMtOPos);
    int32_t *rid = reinterpret_cast<int32_t *>(lds + kMtORow);
    int32_t *act = reinterpret_cast<int32_t *>(lds + kMtOAct);
    const float *zq = lds + (((nl - 1) & 1) ? kMtOH1 : kMtOH0); // the last layer's output
    if ((int64_t)blockIdx.x * kTrTS >= count) // no tile: an all-zero partial (slopes and loss below)
        for (int p = t; p < net.P; p += kTrThreads) out[p] = 0.0f;
    for (int tile = blockIdx.x; (int64_t)tile * kTrTS < count; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int base = tile * kTrTS, nvalid = count - base < kTrTS ? count - base : kTrTS;
        if (t < kTrTS) {
            int64_t s = t < nvalid ? list[base + t] : 0;
            s = s < 0 ? 0 : (s >= b.n ? b.n - 1 : s);
            int64_t r = b.idx[s];
            r = r < 0 ? 0 : (r >= b.max_size ? b.max_size - 1 : r);
            pos[t] = (int32_t)s;
            rid[t] = (int32_t)r;
        }
        __syncthreads();
        // target network on the next states: y = r + gamma max_a Q'(s', a); y = r where done (train.py:121-134)
        mt_forward<false>(net, tgt, b.next_feat, pos, nvalid, lds, nullptr, t, wave, lane);
        if (t < kTrTS) {
            float y = 0.0f;
            int a = 0;
            if (t < nvalid) {
                const int64_t r = rid[t];
                float m = zq[t];
                for (int j = 1; j < n_out; j++) m = fmaxf(m, zq[j * kTrSP + t]);
                const float rew = b.rewards[r * b.A + agent];
                y = b.dones[r] ? rew : rew + gamma * m;
                a = (int)b.actions[r * b.A + agent];
                a = a < 0 ? 0 : (a >= n_out ? n_out - 1 : a);
            }
            lds[kMtOY + t] = y;
            act[t] = a;
        }
        __syncthreads();
        // online network on the states, hidden pre-activations kept in the slice
        mt_forward<true>(net, prm, b.feat, pos, nvalid, lds, zsave, t, wave, lane);
        { // dL/dQ (rows n_out) into the last layer's dZ buffer: 2 (Q - y) / n at the taken action, 0 elsewhere and on padding columns
            float *dq = lds + (((nl - 1) & 1) ? kMtODA : kMtODB);
            for (int e = t; e < n_out * kTrTS; e += kTrThreads) {
                const int j = e / kTrTS, s = e % kTrTS;
                float g = 0.0f;
                if (s < nvalid && j == act[s]) g = inv_n * (zq[j * kTrSP + s] - lds[kMtOY + s]);
                dq[j * kTrSP + s] = g;
            }
            if (t < nvalid) {
                const float diff = zq[act[t] * kTrSP + t] - lds[kMtOY + t];
                lacc += diff * diff;
            }
        }
        __syncthreads();
        // backward, last layer .. first: dz of layer l in DA (l odd) or DB (l even), dh into the other
#pragma unroll
        for (int l = kMtMaxLayers - 1; l >= 0; l--) {
            if (l < nl) {
                const float *dz = lds + ((l & 1) ? kMtODA : kMtODB);
                float *dh = lds + ((l & 1) ? kMtODB : kMtODA);
                float *zin = lds + ((l & 1) ? kMtOH0 : kMtOH1); // the pre-activations of layer l's input (l > 0)
                const int dk = net.d[l], dn = net.d[l + 1];
                float slope_in = 1.0f;
                if (l > 0) {
                    slope_in = prm[net.oA[l > 0 ? l - 1 : 0]];
                    const float *src = zsave + net.zo[l > 0 ? l - 1 : 0];
                    for (int e = t; e < dk * kTrTS; e += kTrThreads) zin[(e >> 5) * kTrSP + (e & 31)] = src[e];
                    __syncthreads();
                }
                // weight gradient of layer l, tile by tile: dW[n][k] += sum_s dz[n][s] h_in[k][s]
                const int KT = (dk + 31) / 32, tiles = ((dn + 31) / 32) * KT;
                for (int g = wave; g < tiles; g += kTrWaves) {
                    const int n0 = (g / KT) * 32, k0 = (g % KT) * 32;
                    const int k = k0 + (lane & 31), kc = k < dk ? k : dk - 1;
                    tr_f32x16 acc = {};
                    acc = tr_mfma([&](int i, int p) { return n0 + i < dn ? dz[(n0 + i) * kTrSP + p] : 0.0f; },
                                  [&](int p, int j) {
                                      if (l == 0) {
                                          const float x = b.feat[(size_t)pos[p] * F + kc];
                                          return (k < dk && p < nvalid) ? x : 0.0f;
                                      }
                                      const float z = zin[kc * kTrSP + p];
                                      return k < dk ? tr_prelu(z, slope_in) : 0.0f;
                                  },
                                  kTrTS, acc, lane);
                    float *wg = out + net.oW[l];
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int n = n0 + tr_row(r, lane);
                        if (n < dn && k < dk) {
                            float *w = wg + (size_t)n * dk + k;
                            *w = first ? acc[r] : *w + acc[r];
                        }
                    }
                }
                if (t < dn) { // bias gradient
                    float s = 0.0f;
                    for (int j = 0; j < kTrTS; j++) s += dz[t * kTrSP + j];
                    float *w = out + net.oB[l] + t;
                    *w = first ? s : *w + s;
                }
                if (l > 0) {
                    tr_backward_layer(prm + net.oW[l], dk, dn, dz, dh, wave, lane);
                    __syncthreads();
                    // through the PReLU of layer l's input: dz = z > 0 ? dh : a dh; d slope = sum over z <= 0 of z dh (torch's prelu backward)
                    for (int e = t; e < dk * kTrTS; e += kTrThreads) {
                        const int k = e / kTrTS, s = e % kTrTS;
                        const float z = zin[k * kTrSP + s], g = dh[k * kTrSP + s];
                        const bool pz = z > 0.0f;
                        dh[k * kTrSP + s] = pz ? g : slope_in * g;
                        sacc[l > 0 ? l - 1 : 0] += pz ? 0.0f : z * g;
                    }
                }
                __syncthreads();
            }
        }
    }
    // slopes and loss: fixed-shape tree sums over the workgroup
    float *red = lds;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMtMaxLayers; q++) {
        if (q < nl) { // q < nl - 1: the slope behind layer q; q == nl - 1: the loss
            tr_block_sum(q < nl - 1 ? sacc[q < 6 ? q : 5] : lacc, red, t);
            if (t == 0) out[q < nl - 1 ? net.oA[q < 6 ? q : 5] : net.P] = red[0];
            __syncthreads();
        }
    }
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

} // namespace susnet
