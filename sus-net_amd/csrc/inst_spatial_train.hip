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
    const int tid = threadIdx.x;
    const int count = counts[2 * agent + team];
    if (count == 0) return;
    const SpTrainNet &net = *netp;
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    const int64_t nimg = (int64_t)count * net.T;
    float *slice = ws.tact + (size_t)blockIdx.x * 2 * net.maxsz;
    for (int64_t job = blockIdx.x; job < 2 * nimg; job += gridDim.x) {
        const bool target = job >= nimg;
        const int64_t img = target ? job - nimg : job;
        const int64_t j = img / net.T;
        const int step = (int)(img % net.T);
        const int64_t s = st_clamp(list[j], b.n);
        const float *P = target ? tgt : prm;
        const float *in = (target ? b.next_spatial : b.spatial) + s * b.sp_stride[0] + agent * b.sp_stride[1] + step * b.sp_stride[2];
        float *xrow = (target ? ws.Xt : ws.X) + (size_t)img * net.R;
        for (int l = 0; l < net.n_conv; l++) {
            float *out = l == net.n_conv - 1 ? xrow : (target ? slice + (l & 1) * net.maxsz : ws.act + (size_t)img * net.asz + net.aoff[l]);
            const int si = net.size[l], so = net.size[l + 1], ci_n = net.ch[l], k = net.k, str = net.stride[l], pad = net.pad[l], dil = net.dil[l];
            const float *W = P + net.oCW[l], *B = P + net.oCB[l];
            for (int e = tid; e < net.sz[l + 1]; e += kStConvThreads) {
                const int co = e / (so * so), oy = (e / so) % so, ox = e % so;
                float acc = B[co];
                for (int ci = 0; ci < ci_n; ci++)
                    for (int ky = 0; ky < k; ky++) {
                        const int iy = oy * str - pad + ky * dil;
                        if (iy < 0 || iy >= si) continue;
                        for (int kx = 0; kx < k; kx++) {
                            const int ix = ox * str - pad + kx * dil;
                            if (ix < 0 || ix >= si) continue;
                            acc = fmaf(W[((co * ci_n + ci) * k + ky) * k + kx], in[(ci * si + iy) * si + ix], acc);
                        }
                    }
                out[e] = acc > 0.0f ? acc : 0.0f;
            }
            __syncthreads();
            in = out;
        }
        if (net.Fn > 0) {
            const float *ns = (target ? b.next_non_spatial : b.non_spatial) + s * b.ns_stride[0] + agent * b.ns_stride[1] + step * b.ns_stride[2];
            for (int f = tid; f < net.Fn; f += kStConvThreads) xrow[net.Rc + f] = ns[f];
        }
    }
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
    const int tid = threadIdx.x;
    const int count = counts[2 * agent + team];
    if (count == 0) return;
    const SpTrainNet &net = *netp;
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    const int64_t nimg = (int64_t)count * net.T;
    float *out = partial + (size_t)blockIdx.x * net.Pp;
    const int k = net.k, last = net.n_conv - 1;
    // through the ReLUs and the transposed convolutions, top down; the gated gradient of every layer's output stays in the workspace
    for (int64_t img = blockIdx.x; img < nimg; img += gridDim.x) {
        for (int l = last; l >= 0; l--) {
            const float *y = l == last ? ws.X + (size_t)img * net.R : ws.act + (size_t)img * net.asz + net.aoff[l];
            float *d = l == last ? ws.dX + (size_t)img * net.Rc : ws.dact + (size_t)img * net.asz + net.aoff[l];
            for (int e = tid; e < net.sz[l + 1]; e += kStConvThreads) d[e] = y[e] > 0.0f ? d[e] : 0.0f; // relu'(0) = 0, as torch
            __syncthreads();
            if (l > 0) {
                float *din = ws.dact + (size_t)img * net.asz + net.aoff[l > 0 ? l - 1 : 0];
                const int si = net.size[l], so = net.size[l + 1], ci_n = net.ch[l], co_n = net.ch[l + 1], str = net.stride[l], pad = net.pad[l],
                          dil = net.dil[l];
                const float *W = prm + net.oCW[l];
                for (int e = tid; e < net.sz[l]; e += kStConvThreads) {
                    const int ci = e / (si * si), iy = (e / si) % si, ix = e % si;
                    float acc = 0.0f;
                    for (int co = 0; co < co_n; co++)
                        for (int ky = 0; ky < k; ky++) {
                            const int ny = iy + pad - ky * dil;
                            if (ny < 0 || ny % str != 0 || ny / str >= so) continue;
                            for (int kx = 0; kx < k; kx++) {
                                const int nx = ix + pad - kx * dil;
                                if (nx < 0 || nx % str != 0 || nx / str >= so) continue;
                                acc = fmaf(W[((co * ci_n + ci) * k + ky) * k + kx], d[(co * so + ny / str) * so + nx / str], acc);
                            }
                        }
                    din[e] = acc;
                }
                __syncthreads();
            }
        }
    }
    // weight and bias gradients: a thread per parameter, images then pixels in ascending order, stored once
    for (int l = 0; l <= last; l++) {
        const int si = net.size[l], so = net.size[l + 1], ci_n = net.ch[l], co_n = net.ch[l + 1], str = net.stride[l], pad = net.pad[l], dil = net.dil[l];
        const int nW = co_n * ci_n * k * k;
        for (int w = tid; w < nW + co_n; w += kStConvThreads) {
            const bool bias = w >= nW;
            const int co = bias ? w - nW : w / (ci_n * k * k), ci = bias ? 0 : (w / (k * k)) % ci_n, ky = bias ? 0 : (w / k) % k, kx = bias ? 0 : w % k;
            float acc = 0.0f;
            for (int64_t img = blockIdx.x; img < nimg; img += gridDim.x) {
                const float *d = (l == last ? ws.dX + (size_t)img * net.Rc : ws.dact + (size_t)img * net.asz + net.aoff[l]) + (size_t)co * so * so;
                if (bias) {
                    for (int e = 0; e < so * so; e++) acc += d[e];
                    continue;
                }
                const float *in;
                if (l == 0) {
                    const int64_t s = st_clamp(list[img / net.T], b.n);
                    in = b.spatial + s * b.sp_stride[0] + agent * b.sp_stride[1] + (img % net.T) * b.sp_stride[2];
                } else {
                    in = ws.act + (size_t)img * net.asz + net.aoff[l > 0 ? l - 1 : 0];
                }
                in += (size_t)ci * si * si;
                for (int oy = 0; oy < so; oy++) {
                    const int iy = oy * str - pad + ky * dil;
                    if (iy < 0 || iy >= si) continue;
                    for (int ox = 0; ox < so; ox++) {
                        const int ix = ox * str - pad + kx * dil;
                        if (ix < 0 || ix >= si) continue;
                        acc = fmaf(d[oy * so + ox], in[iy * si + ix], acc);
                    }
                }
            }
            out[bias ? net.oCB[l] + co : net.oCW[l] + w] = acc;
        }
    }
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
