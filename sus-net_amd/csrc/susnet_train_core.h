// susnet_train_core.h -- what the two DQN learners share (susnet_train.h: the fused learner on the compiled-in feature layouts;
// susnet_mlp_train.h / inst_mlp_train.hip: the dense learner on any served stack): the tile constants, the matrix-product and layer
// device functions, the row selection, the workgroup sum that closes both gradient kernels, Adam, and the host-side layout of the
// parameters and of the workspace.  Device FUNCTIONS only -- no kernel is defined here, so any unit may include it; every function is
// inlined into the kernels that call it, each of which is bitwise reproducible: no atomics, every sum in a fixed order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace susnet {

typedef float tr_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTrThreads = 512, kTrWaves = kTrThreads / 64, kTrTS = 32, kTrSP = 33; // threads; waves; rows of a tile; LDS row stride (floats)

__device__ __forceinline__ float tr_prelu(float z, float a) { return z > 0.0f ? z : a * z; } // torch.prelu

// D[i][j] (+)= sum_p A(i, p) B(p, j) for one 32 x 32 tile, K steps of 2 on v_mfma_f32_32x32x2_f32: lane l feeds A(l % 32, p0 + l / 32)
// and B(p0 + l / 32, l % 32); register r of the result is row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32.
template <class FA, class FB>
__device__ __forceinline__ tr_f32x16 tr_mfma(FA fa, FB fb, int K, tr_f32x16 acc, int lane) {
    const int i = lane & 31, h = lane >> 5;
    for (int p0 = 0; p0 < K; p0 += 2) {
        const int p = p0 + h;
        const float a = p < K ? fa(i, p) : 0.0f, b = p < K ? fb(p, i) : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ int tr_row(int r, int lane) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }

// forward of layer l (0-based): Z_out[n][s] = b[n] + sum_k W[n][k] h_in[k][s], h_in = X (l = 0) or prelu(Z_in)
__device__ __forceinline__ void tr_forward_layer(const float *__restrict__ W, const float *__restrict__ bias, int dk, int dn, const float *zin, float slope_in,
                                                 bool raw_in, float *zout, int wave, int lane) {
    const int nt_count = (dn + 31) / 32;
    for (int nt = wave; nt < nt_count; nt += kTrWaves) {
        const int n0 = nt * 32;
        tr_f32x16 acc = {};
        acc = tr_mfma([&](int i, int p) { return n0 + i < dn ? W[(size_t)(n0 + i) * dk + p] : 0.0f; },
                      [&](int p, int j) { const float z = zin[p * kTrSP + j]; return raw_in ? z : tr_prelu(z, slope_in); }, dk, acc, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int n = n0 + tr_row(r, lane);
            if (n < dn) zout[n * kTrSP + (lane & 31)] = acc[r] + bias[n];
        }
    }
}

// backward through layer l: dH_in[k][s] = sum_n W[n][k] dZ[n][s]
__device__ __forceinline__ void tr_backward_layer(const float *__restrict__ W, int dk, int dn, const float *dz, float *dh, int wave, int lane) {
    const int kt_count = (dk + 31) / 32;
    for (int kt = wave; kt < kt_count; kt += kTrWaves) {
        const int k0 = kt * 32;
        tr_f32x16 acc = {};
        acc = tr_mfma([&](int i, int p) { return k0 + i < dk ? W[(size_t)p * dk + k0 + i] : 0.0f; }, [&](int p, int j) { return dz[p * kTrSP + j]; }, dn,
                      acc, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int k = k0 + tr_row(r, lane);
            if (k < dk) dh[k * kTrSP + (lane & 31)] = acc[r];
        }
    }
}

// the team's rows of one agent: ring row ids, stable order
__device__ __forceinline__ int32_t *tr_list(int32_t *lists, int64_t N, int agent, int team) { return lists + ((int64_t)agent * 2 + team) * N; }

// ---- the select kernels' body: ONE workgroup of kTrThreads (per learner) splits the N sampled rows into a stable list per (agent, team)
// -- imposter rows = imposters[row, 0] == agent -- with its count, and zeroes the gradient accumulators and the two losses.  The lists hold
// ring rows (the fused learner reads the ring in place), or -- POS -- batch positions s, whose ring row is clamp(idx[s]) (the dense learner:
// the positions index its feature rows).  Of RING (TrainRing / MlpTrainBatch) it reads imposters, n_imp, max_size and A, where it uses them ----
template <bool POS, class RING>
__device__ __forceinline__ void tr_select(const RING &ring, const int64_t *__restrict__ idx, int64_t N, int32_t *lists, int32_t *counts, float *gacc0,
                                          int P0, float *gacc1, int P1, float *losses, int32_t *tr_scan) {
    const int t = threadIdx.x;
    for (int p = t; p < P0; p += kTrThreads) gacc0[p] = 0.0f;
    for (int p = t; p < P1; p += kTrThreads) gacc1[p] = 0.0f;
    if (t < 2) losses[t] = 0.0f;
    const int64_t chunk = (N + kTrThreads - 1) / kTrThreads, lo = (int64_t)t * chunk, hi = lo + chunk < N ? lo + chunk : N;
    for (int agent = 0; agent < ring.A; agent++) {
        int32_t c = 0;
        for (int64_t s = lo; s < hi; s++) {
            int64_t r = idx[s];
            r = r < 0 ? 0 : (r >= ring.max_size ? ring.max_size - 1 : r);
            c += (int)ring.imposters[r * ring.n_imp] == agent ? 1 : 0;
        }
        tr_scan[t] = c;
        __syncthreads();
        for (int off = 1; off < kTrThreads; off <<= 1) { // inclusive Hillis-Steele scan
            const int32_t v = t >= off ? tr_scan[t - off] : 0;
            __syncthreads();
            tr_scan[t] += v;
            __syncthreads();
        }
        const int32_t total = tr_scan[kTrThreads - 1];
        int32_t pi = tr_scan[t] - c;                       // imposter rows before this chunk
        int32_t pc = (int32_t)(lo < N ? lo : N) - pi;        // crew rows before this chunk
        int32_t *li = tr_list(lists, N, agent, 0), *lc = tr_list(lists, N, agent, 1);
        for (int64_t s = lo; s < hi; s++) {
            int64_t r = idx[s];
            r = r < 0 ? 0 : (r >= ring.max_size ? ring.max_size - 1 : r);
            if ((int)ring.imposters[r * ring.n_imp] == agent) li[pi++] = (int32_t)(POS ? s : r);
            else lc[pc++] = (int32_t)(POS ? s : r);
        }
        if (t == 0) {
            counts[2 * agent] = total;
            counts[2 * agent + 1] = (int32_t)N - total;
        }
        __syncthreads();
    }
}

// ---- the gradient kernels' closing sums: the workgroup's kTrThreads values of v, added as a fixed-shape tree (red[t] += red[t + off],
// off = kTrThreads / 2 .. 1: bitwise reproducible).  The sum is left in red[0], behind a barrier: every thread may read it, and the caller
// puts a barrier before red is written again.  red: kTrThreads floats of LDS nobody reads any more (a barrier precedes the call).
// (minsize keeps the loop rolled until the function is inlined; the kernel then unrolls it together with its own loops, as it did when
// the loop stood in the kernel -- unrolled here first, k_mlp_train_grad comes out as different machine code than the one that was measured) ----
__device__ __forceinline__ __attribute__((minsize)) void tr_block_sum(float v, float *red, int t) {
    red[t] = v;
    __syncthreads();
    for (int off = kTrThreads / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
}

// ---- the Adam kernels' body: thread per parameter of a stack of P parameters whose partials have stride Pp ----
__device__ __forceinline__ void tr_adam(int P, int Pp, const int32_t *__restrict__ counts, int agent, int team, const float *__restrict__ partial, int G,
                                        float *__restrict__ gacc, float *__restrict__ prm, float *__restrict__ m1, float *__restrict__ m2,
                                        const float *__restrict__ step, double lr, double beta1, double beta2, double eps, float *losses) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int count = counts[2 * agent + team];
    if (count == 0 || p > P) return; // an empty team takes no step (train.py:101)
    float g = 0.0f;
    for (int w = 0; w < G; w++) g += partial[(size_t)w * Pp + p];
    if (p == P) { // F.mse_loss (mean) of this update, summed over agents (train.py:139)
        losses[team] += g / (float)count;
        return;
    }
    const float ga = gacc[p] + g; // loss.backward() accumulates into .grad (zero_grad once per call, train.py:64-67)
    gacc[p] = ga;
    // torch.optim.adam._single_tensor_adam: lerp, mul + addcmul, bias corrections in double, sqrt(v) / sqrt(bc2) + eps, addcdiv
    const double st = (double)step[0];
    const float b1w = (float)(1.0 - beta1);
    float m = m1[p];
    m = m + b1w * (ga - m);
    float v = m2[p];
    v = v * (float)beta2 + (float)(1.0 - beta2) * (ga * ga);
    m1[p] = m;
    m2[p] = v;
    const double bc1 = 1.0 - pow(beta1, st), bc2 = 1.0 - pow(beta2, st);
    const float step_size = (float)(lr / bc1), bc2s = (float)sqrt(bc2);
    const float denom = sqrtf(v) / bc2s + (float)eps;
    prm[p] = prm[p] + (-step_size) * (m / denom);
}

// ---- host side: the layouts both learners' plans share ----
// parameter offsets of an nl-layer stack net.d[0 .. nl] in MLP.parameters() order -- Linear weight, Linear bias, PReLU weight, ...
// (dqn.py:322-329) --, the parameter count P and the partial stride Pp = P + 1 (the loss sum), rounded up to 4.  NET: TrainNet / MlpTrainNet
template <class NET>
inline void tr_param_layout(NET &net, int nl) {
    int off = 0;
    for (int l = 0; l < nl; l++) {
        net.oW[l] = off;
        off += net.d[l + 1] * net.d[l];
        net.oB[l] = off;
        off += net.d[l + 1];
        if (l < nl - 1) net.oA[l] = off++;
    }
    net.P = off;
    net.Pp = (off + 1 + 3) / 4 * 4;
}
// the workspace both train steps start with, every part 256-byte aligned: the 2 A lists of n rows, their counts, a gradient accumulator per
// team, the G workgroups' partials of stride pmax.  Returns the bytes so far: what a learner keeps beyond these goes behind them.
struct TrWorkspace {
    uint64_t off_lists = 0, off_counts = 0, off_gacc[2] = {0, 0}, off_partial = 0;
};
inline uint64_t tr_workspace_layout(TrWorkspace &w, int A, int64_t n, int Pp0, int Pp1, int64_t G, int64_t pmax) {
    const auto up256 = [](uint64_t v) { return (v + 255) / 256 * 256; };
    const int Pp[2] = {Pp0, Pp1};
    uint64_t o = 0;
    w.off_lists = o;
    o = up256(o + 4ull * 2 * A * (uint64_t)(n > 1 ? n : 1));
    w.off_counts = o;
    o = up256(o + 4ull * 2 * A);
    for (int tm = 0; tm < 2; tm++) {
        w.off_gacc[tm] = o;
        o = up256(o + 4ull * (uint64_t)(Pp[tm] > 4 ? Pp[tm] : 4));
    }
    w.off_partial = o;
    return up256(o + 4ull * (uint64_t)G * (uint64_t)pmax);
}

} // namespace susnet
