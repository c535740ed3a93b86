// the SpatialDQN learner's kernels (susnet_spatial_train.h: susnet_spatial_train_step) -- a translation unit of its own
#include "susnet_spatial_train.h"

#include "susnet_host.h" // lds_opt_in
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

// tanh as susnet_spatial_forward computes it (inst_qnet_spatial.hip, sp_tanh): exactly 0 at 0, exactly +-1 from |x| = 16
__device__ __forceinline__ float st_tanh(float x) {
    const float ax = fabsf(x);
    const float e = expm1f(-2.0f * ax);
    const float t = ax >= 16.0f ? 1.0f : -e / (e + 2.0f);
    return copysignf(t, x);
}

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
__device__ __forceinline__ void st_rnn_step(const SpTrainNet &net, const float *__restrict__ P, int l, int t, const float *X, int64_t j0, int nvalid,
                                            float *hs, int wave, int lane) {
    const int H = net.H, R = net.R, T = net.T, s = lane & 31;
    const bool svalid = s < nvalid;
    const float *Wih = P + net.oWih[l], *Whh = P + net.oWhh[l], *bih = P + net.oBih[l], *bhh = P + net.oBhh[l];
    const float *xrow = X + ((size_t)(j0 + (svalid ? s : 0)) * T + t) * R;
    const float *hin = hs + ((size_t)((l > 0 ? l - 1 : 0) * T + t) * H) * kTrTS;
    const float *hprev = hs + ((size_t)(l * T + (t > 0 ? t - 1 : 0)) * H) * kTrTS;
    float *hout = hs + ((size_t)(l * T + t) * H) * kTrTS;
    const int nt_count = (H + 31) / 32;
    for (int nt = wave; nt < nt_count; nt += kTrWaves) {
        const int n0 = nt * 32;
        tr_f32x16 acc = {};
        if (l == 0)
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Wih[(size_t)(n0 + i) * R + p] : 0.0f; },
                          [&](int p, int j) { return svalid ? xrow[p] : 0.0f; }, R, acc, lane);
        else
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Wih[(size_t)(n0 + i) * H + p] : 0.0f; },
                          [&](int p, int j) { return hin[p * kTrTS + j]; }, H, acc, lane);
        if (t > 0)
            acc = tr_mfma([&](int i, int p) { return n0 + i < H ? Whh[(size_t)(n0 + i) * H + p] : 0.0f; },
                          [&](int p, int j) { return hprev[p * kTrTS + j]; }, H, acc, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int n = n0 + tr_row(r, lane);
            if (n < H) hout[n * kTrTS + s] = st_tanh(acc[r] + (bih[n] + bhh[n]));
        }
    }
}

// the whole network behind the convolutions on one tile: recurrence into hs, then the head on LDS (layer l writes buffer l & 1; layer 0
// reads the top layer's last hidden state, copied into buffer 1).  SAVE: the head's hidden pre-activations also go to zsave, as
// inst_mlp_train.hip's mt_forward keeps them
template <bool SAVE>
__device__ __forceinline__ void st_forward(const SpTrainNet &net, const float *__restrict__ P, const float *X, int64_t j0, int nvalid, float *hs,
                                           float *lds, float *zsave, int tid, int wave, int lane) {
    for (int t = 0; t < net.T; t++)
        for (int l = 0; l < net.L; l++) {
            st_rnn_step(net, P, l, t, X, j0, nvalid, hs, wave, lane);
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
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int count = counts[2 * agent + team];
    if (count == 0) return; // an empty team takes no step (train.py:101): k_train_adam does nothing either
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    if (blockIdx.x == 0 && tid == 0) step[0] += 1.0f; // (k_train_adam reads it after this launch)
    const SpTrainNet &net = *netp;
    const MlpTrainNet &hd = net.head;
    const int nl = hd.nl, n_out = hd.d[nl], H = net.H, L = net.L, T = net.T, R = net.R, Rc = net.Rc;
    float *out = partial + (size_t)blockIdx.x * net.Pp;
    const size_t slice = (size_t)L * T * H * kTrTS;
    float *hs = ws.hs + (size_t)blockIdx.x * slice, *ds = ws.ds + (size_t)blockIdx.x * slice;
    float *zsave = ws.zs + (size_t)blockIdx.x * hd.Z;
    float lacc = 0.0f;
    float *red = lds + kStORed;
    const float inv_n = 2.0f / (float)count; // mse_loss backward: 2 (x - y) / numel
    int32_t *rid = reinterpret_cast<int32_t *>(lds + kStORow);
    int32_t *act = reinterpret_cast<int32_t *>(lds + kStOAct);
    const float *zq = lds + (((nl - 1) & 1) ? kStOH1 : kStOH0); // the last layer's output
    if ((int64_t)blockIdx.x * kTrTS >= count) // no tile: an all-zero partial behind the convolutions' part (slopes and loss below)
        for (int p = net.oWih[0] + tid; p < net.P; p += kTrThreads) out[p] = 0.0f;
    for (int tile = blockIdx.x; (int64_t)tile * kTrTS < count; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int base = tile * kTrTS, nvalid = count - base < kTrTS ? count - base : kTrTS;
        const int64_t j0 = base;
        if (tid < kTrTS) {
            const int64_t s = st_clamp(tid < nvalid ? list[base + tid] : 0, b.n);
            rid[tid] = (int32_t)st_clamp(b.idx[s], b.max_size);
        }
        __syncthreads();
        // target network on the next states: y = r + gamma max_a Q'(s', a); y = r where done (train.py:121-134)
        st_forward<false>(net, tgt, ws.Xt, j0, nvalid, hs, lds, nullptr, tid, wave, lane);
        if (tid < kTrTS) {
            float y = 0.0f;
            int a = 0;
            if (tid < nvalid) {
                const int64_t r = rid[tid];
                float m = zq[tid];
                for (int j = 1; j < n_out; j++) m = fmaxf(m, zq[j * kTrSP + tid]);
                const float rew = b.rewards[r * b.A + agent];
                y = b.dones[r] ? rew : rew + gamma * m;
                a = (int)b.actions[r * b.A + agent];
                a = a < 0 ? 0 : (a >= n_out ? n_out - 1 : a);
            }
            lds[kStOY + tid] = y;
            act[tid] = a;
        }
        __syncthreads();
        // online network on the states: every h[l][t] in hs, the head's hidden pre-activations in zsave
        st_forward<true>(net, prm, ws.X, j0, nvalid, hs, lds, zsave, tid, wave, lane);
        { // dL/dQ into the last layer's dZ buffer: 2 (Q - y) / n at the taken action, 0 elsewhere and on padding columns
            float *dq = lds + (((nl - 1) & 1) ? kStODA : kStODB);
            for (int e = tid; e < n_out * kTrTS; e += kTrThreads) {
                const int j = e / kTrTS, s = e % kTrTS;
                float g = 0.0f;
                if (s < nvalid && j == act[s]) g = inv_n * (zq[j * kTrSP + s] - lds[kStOY + s]);
                dq[j * kTrSP + s] = g;
            }
            if (tid < nvalid) {
                const float diff = zq[act[tid] * kTrSP + tid] - lds[kStOY + tid];
                lacc += diff * diff;
            }
        }
        __syncthreads();
        // the head's backward, last layer .. first, as k_mlp_train_grad: dz of layer l in DA (l odd) or DB (l even), dh into the other;
        // layer 0's input is the top hidden state (no activation in front of it), and its dh -- left in DA -- is the recurrence's
        for (int l = nl - 1; l >= 0; l--) {
            {
                const float *dz = lds + ((l & 1) ? kStODA : kStODB);
                float *dh = lds + ((l & 1) ? kStODB : kStODA);
                float *zin = lds + ((l & 1) ? kStOH0 : kStOH1);
                const int dk = hd.d[l], dn = hd.d[l + 1];
                const float slope_in = l > 0 ? prm[hd.oA[l - 1]] : 1.0f;
                {
                    const float *src = l > 0 ? zsave + hd.zo[l - 1] : hs + ((size_t)((L - 1) * T + T - 1) * H) * kTrTS;
                    for (int e = tid; e < dk * kTrTS; e += kTrThreads) zin[(e >> 5) * kTrSP + (e & 31)] = src[e];
                    __syncthreads();
                }
                const int KT = (dk + 31) / 32, tiles = ((dn + 31) / 32) * KT;
                for (int g = wave; g < tiles; g += kTrWaves) {
                    const int n0 = (g / KT) * 32, k0 = (g % KT) * 32;
                    const int k = k0 + (lane & 31), kc = k < dk ? k : dk - 1;
                    tr_f32x16 acc = {};
                    acc = tr_mfma([&](int i, int p) { return n0 + i < dn ? dz[(n0 + i) * kTrSP + p] : 0.0f; },
                                  [&](int p, int j) {
                                      const float z = zin[kc * kTrSP + p];
                                      return k < dk ? (l == 0 ? z : tr_prelu(z, slope_in)) : 0.0f;
                                  },
                                  kTrTS, acc, lane);
                    float *wg = out + hd.oW[l];
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int n = n0 + tr_row(r, lane);
                        if (n < dn && k < dk) {
                            float *w = wg + (size_t)n * dk + k;
                            *w = first ? acc[r] : *w + acc[r];
                        }
                    }
                }
                if (tid < dn) { // bias gradient
                    float s = 0.0f;
                    for (int j = 0; j < kTrTS; j++) s += dz[tid * kTrSP + j];
                    float *w = out + hd.oB[l] + tid;
                    *w = first ? s : *w + s;
                }
                tr_backward_layer(prm + hd.oW[l], dk, dn, dz, dh, wave, lane);
                __syncthreads();
                if (l > 0) { // through the PReLU of layer l's input (torch's prelu backward); the slope's gradient: a fixed-shape tree sum per tile
                    float sl = 0.0f;
                    for (int e = tid; e < dk * kTrTS; e += kTrThreads) {
                        const int k = e / kTrTS, s = e % kTrTS;
                        const float z = zin[k * kTrSP + s], g = dh[k * kTrSP + s];
                        const bool pz = z > 0.0f;
                        dh[k * kTrSP + s] = pz ? g : slope_in * g;
                        sl += pz ? 0.0f : z * g;
                    }
                    tr_block_sum(sl, red, tid);
                    if (tid == 0) {
                        float *w = out + hd.oA[l - 1];
                        *w = first ? red[0] : *w + red[0];
                    }
                    __syncthreads();
                }
            }
        }
        const float *dhead = lds + kStODA; // [H][kTrSP]
        // back through time: dz[l][t] = (1 - h^2) (W_ih[l+1]^T dz[l+1][t] + W_hh[l]^T dz[l][t+1] (+ dhead at the top, last step))
        const int kt_count = (H + 31) / 32;
        for (int t = T - 1; t >= 0; t--) {
            for (int l = L - 1; l >= 0; l--) {
                const float *Wup = prm + net.oWih[l < L - 1 ? l + 1 : l], *Whh = prm + net.oWhh[l];
                const float *dzup = ds + ((size_t)((l < L - 1 ? l + 1 : l) * T + t) * H) * kTrTS;
                const float *dzfut = ds + ((size_t)(l * T + (t < T - 1 ? t + 1 : t)) * H) * kTrTS;
                const float *h = hs + ((size_t)(l * T + t) * H) * kTrTS;
                float *dzo = ds + ((size_t)(l * T + t) * H) * kTrTS;
                const bool top = l == L - 1 && t == T - 1;
                for (int kt = wave; kt < kt_count; kt += kTrWaves) {
                    const int k0 = kt * 32;
                    tr_f32x16 acc = {};
                    if (l < L - 1)
                        acc = tr_mfma([&](int i, int p) { return k0 + i < H ? Wup[(size_t)p * H + k0 + i] : 0.0f; },
                                      [&](int p, int j) { return dzup[p * kTrTS + j]; }, H, acc, lane);
                    if (t < T - 1)
                        acc = tr_mfma([&](int i, int p) { return k0 + i < H ? Whh[(size_t)p * H + k0 + i] : 0.0f; },
                                      [&](int p, int j) { return dzfut[p * kTrTS + j]; }, H, acc, lane);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int k = k0 + tr_row(r, lane), s = lane & 31;
                        if (k < H) {
                            const float g = acc[r] + (top ? dhead[k * kTrSP + s] : 0.0f);
                            const float hv = h[k * kTrTS + s];
                            dzo[k * kTrTS + s] = (1.0f - hv * hv) * g;
                        }
                    }
                }
                __syncthreads();
            }
        }
        { // gradient of the RNN input's convolution columns: dX[s][t][k] = sum_n W_ih[0][n][k] dz[0][t][n][s], k < Rc
            const float *W0 = prm + net.oWih[0];
            const int KT = (Rc + 31) / 32;
            for (int g = wave; g < T * KT; g += kTrWaves) {
                const int t = g / KT, k0 = (g % KT) * 32;
                const float *dz0 = ds + ((size_t)t * H) * kTrTS;
                tr_f32x16 acc = {};
                acc = tr_mfma([&](int i, int p) { return k0 + i < Rc ? W0[(size_t)p * R + k0 + i] : 0.0f; }, [&](int p, int j) { return dz0[p * kTrTS + j]; },
                              H, acc, lane);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int k = k0 + tr_row(r, lane), s = lane & 31;
                    if (k < Rc && s < nvalid) ws.dX[((size_t)(j0 + s) * T + t) * Rc + k] = acc[r];
                }
            }
        }
        // the recurrence's weight gradients, one product over all steps and the tile's rows per 32 x 32 block: p = 32 t + s
        for (int l = 0; l < L; l++) {
            const int dk = l == 0 ? R : H;
            const float *dzl = ds + ((size_t)(l * T) * H) * kTrTS;
            const float *hbelow = hs + ((size_t)((l > 0 ? l - 1 : 0) * T) * H) * kTrTS;
            const float *hown = hs + ((size_t)(l * T) * H) * kTrTS;
            const int KT = (dk + 31) / 32, HT = (H + 31) / 32;
            for (int g = wave; g < HT * KT; g += kTrWaves) { // dW_ih[n][k] = sum_{t, s} dz[l][t][n][s] in[l][t][k][s]
                const int n0 = (g / KT) * 32, k0 = (g % KT) * 32;
                const int k = k0 + (lane & 31), kc = k < dk ? k : dk - 1;
                tr_f32x16 acc = {};
                acc = tr_mfma([&](int i, int p) { return n0 + i < H ? dzl[((size_t)(p >> 5) * H + n0 + i) * kTrTS + (p & 31)] : 0.0f; },
                              [&](int p, int j) {
                                  const int t = p >> 5, s = p & 31;
                                  float x;
                                  if (l == 0) x = s < nvalid ? ws.X[((size_t)(j0 + (s < nvalid ? s : 0)) * T + t) * R + kc] : 0.0f;
                                  else x = hbelow[((size_t)t * H + kc) * kTrTS + s];
                                  return k < dk ? x : 0.0f;
                              },
                              T * kTrTS, acc, lane);
                float *wg = out + net.oWih[l];
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = n0 + tr_row(r, lane);
                    if (n < H && k < dk) {
                        float *w = wg + (size_t)n * dk + k;
                        *w = first ? acc[r] : *w + acc[r];
                    }
                }
            }
            for (int g = wave; g < HT * HT; g += kTrWaves) { // dW_hh[n][k] = sum_{t >= 1, s} dz[l][t][n][s] h[l][t-1][k][s]
                const int n0 = (g / HT) * 32, k0 = (g % HT) * 32;
                const int k = k0 + (lane & 31), kc = k < H ? k : H - 1;
                tr_f32x16 acc = {};
                acc = tr_mfma([&](int i, int p) { return n0 + i < H ? dzl[((size_t)((p >> 5) + 1) * H + n0 + i) * kTrTS + (p & 31)] : 0.0f; },
                              [&](int p, int j) {
                                  const float x = hown[((size_t)(p >> 5) * H + kc) * kTrTS + (p & 31)];
                                  return k < H ? x : 0.0f;
                              },
                              (T - 1) * kTrTS, acc, lane);
                float *wg = out + net.oWhh[l];
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = n0 + tr_row(r, lane);
                    if (n < H && k < H) {
                        float *w = wg + (size_t)n * H + k;
                        *w = first ? acc[r] : *w + acc[r];
                    }
                }
            }
            if (tid < H) { // bias_ih and bias_hh: the same gradient
                float s = 0.0f;
                for (int p = 0; p < T * kTrTS; p++) s += dzl[((size_t)(p >> 5) * H + tid) * kTrTS + (p & 31)];
                float *w1 = out + net.oBih[l] + tid, *w2 = out + net.oBhh[l] + tid;
                const float v = first ? s : *w1 + s;
                *w1 = v;
                *w2 = v;
            }
        }
        __syncthreads(); // (the next tile rewrites rid, the slices and the LDS buffers)
    }
    // the loss: a fixed-shape tree sum over the workgroup
    __syncthreads();
    tr_block_sum(lacc, red, tid);
    if (tid == 0) out[net.P] = red[0];
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
                                  int Gconv, hipStream_t st) {
    // the recurrence kernel's dynamic-LDS ceiling, set once per device (not repeated inside a capture after the first eager step)
    static LdsOptIn opted;
    if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_sp_train_rnn), kStLdsBytes, opted)) return e;
    hipLaunchKernelGGL(k_sp_train_conv, dim3((unsigned)Gconv), dim3(kStConvThreads), 0, st, b, net, ws, prm, tgt, lists, counts, agent, team);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_sp_train_rnn, dim3((unsigned)G), dim3(kTrThreads), kStLdsBytes, st, b, net, ws, prm, tgt, lists, counts, agent, team, gamma,
                       partial, step);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_sp_train_conv_bwd, dim3((unsigned)G), dim3(kStConvThreads), 0, st, b, net, ws, prm, lists, counts, agent, team, partial);
    return hipGetLastError();
}

} // namespace susnet
