// the SpatialDQN forward kernels (susnet_spatial.h: susnet_spatial_forward) -- a translation unit of its own, default scheduling like the
// other Q-network units
#include "susnet_spatial.h"

#include "susnet_dropout.h"
#include "susnet_host.h" // lds_opt_in

namespace susnet {

// ---- the convolution stack ------------------------------------------------------------------------------------------------------------
// A parameter read through the constant address space: nothing writes the parameters while the kernel runs, and with a lane-independent
// index the load is a scalar one whose result is the FMA's scalar operand.
typedef const __attribute__((address_space(4))) float *sp_const_ptr;
__device__ __forceinline__ float sp_param(const float *p, int idx) { return ((sp_const_ptr)(uintptr_t)p)[idx]; }

// one Conv2d + ReLU layer of a group's `cnt` images: lane -> (image g, output pixel p), all Co <= CB output channels in registers
template <int CB, int K>
__device__ __forceinline__ void sp_conv_layer(const float *__restrict__ W, const float *__restrict__ bias, int Ci, int Co, int Hi, int Ho, int stride,
                                              int pad, int dil, const float *in, int slot_in, float *out, int64_t slot_out, int cnt, int tid) {
    const int P = Ho * Ho, items = cnt * P, plane = Hi * Hi;
    for (int it = tid; it < items; it += kSpThreads) {
        const int g = it / P, p = it - g * P, oy = p / Ho, ox = p - oy * Ho;
        float acc[CB];
#pragma unroll
        for (int j = 0; j < CB; j++) acc[j] = sp_param(bias, j < Co ? j : Co - 1);
        // the taps of this pixel: offset inside a channel plane (clamped to 0 for a padding tap) and whether the tap is inside the image
        int off[K * K];
        bool ok[K * K];
#pragma unroll
        for (int ky = 0; ky < K; ky++)
#pragma unroll
            for (int kx = 0; kx < K; kx++) {
                const int iy = oy * stride - pad + ky * dil, ix = ox * stride - pad + kx * dil;
                const bool inside = iy >= 0 && iy < Hi && ix >= 0 && ix < Hi;
                ok[ky * K + kx] = inside;
                off[ky * K + kx] = inside ? iy * Hi + ix : 0;
            }
        const float *src = in + g * slot_in;
        for (int ci = 0; ci < Ci; ci++) {
#pragma unroll
            for (int tap = 0; tap < K * K; tap++) {
                const float xv = src[ci * plane + off[tap]];
                const float x = ok[tap] ? xv : 0.0f;
#pragma unroll
                for (int j = 0; j < CB; j++) { // (wave-uniform weight index: a channel past Co repeats the last one, its result is dropped)
                    const float w = sp_param(W, ((j < Co ? j : Co - 1) * Ci + ci) * (K * K) + tap);
                    acc[j] = fmaf(w, x, acc[j]);
                }
            }
        }
        float *dst = out + g * slot_out + p;
#pragma unroll
        for (int j = 0; j < CB; j++)
            if (j < Co) dst[j * P] = acc[j] <= 0.0f ? 0.0f : acc[j]; // ReLU
    }
}

// CB: the smallest of 4 / 8 / 16 / 32 that holds the stack's widest layer; a layer of at most half that width runs the narrower form
template <int CB, int K>
__global__ __launch_bounds__(kSpThreads) void k_spatial_conv(SpatialConvArgs a) {
    extern __shared__ float sp_smem[];
    const int tid = threadIdx.x;
    const int64_t images = a.n * a.T, groups = (images + a.G - 1) / a.G;
    const int imgsz = a.C * a.size[0] * a.size[0];
    const int last_p = a.size[a.n_conv] * a.size[a.n_conv], conv_cols = a.co[a.n_conv - 1] * last_p;
    float *buf0 = sp_smem, *buf1 = sp_smem + a.G * a.slot0;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t m0 = grp * a.G;
        const int cnt = (int)(images - m0 < a.G ? images - m0 : a.G);
        for (int g = 0; g < cnt; g++) { // image m = row r, window step t; row r = env r / agents, agent r % agents
            const int64_t m = m0 + g, r = m / a.T, t = m - r * a.T, env = r / a.agents, ag = r - env * a.agents;
            const float *img = a.spatial + env * a.sp_stride[0] + ag * a.sp_stride[1] + t * a.sp_stride[2];
            for (int e = tid; e < imgsz; e += kSpThreads) buf0[g * a.slot0 + e] = img[e];
            const float *ns = a.non_spatial + env * a.ns_stride[0] + ag * a.ns_stride[1] + t * a.ns_stride[2];
            float *row = a.rnn_in + m * a.R + conv_cols; // the torch.cat of dqn.py:294: the non-spatial columns follow the flattened planes
            for (int f = tid; f < a.Fn; f += kSpThreads) row[f] = ns[f];
        }
        __syncthreads();
        for (int l = 0; l < a.n_conv; l++) {
            const bool last = l == a.n_conv - 1;
            const float *in = (l & 1) ? buf1 : buf0;
            const int slot_in = (l & 1) ? a.slot1 : a.slot0;
            const int slot_lds = (l & 1) ? a.slot0 : a.slot1;
            float *out_lds = (l & 1) ? buf0 : buf1;
            const int Ci = l == 0 ? a.C : a.co[l - 1], Co = a.co[l];
            float *out = last ? a.rnn_in + m0 * a.R : out_lds;
            const int64_t slot_out = last ? (int64_t)a.R : (int64_t)slot_lds;
            if (CB > 4 && Co <= CB / 2)
                sp_conv_layer<(CB > 4 ? CB / 2 : CB), K>(a.W[l], a.B[l], Ci, Co, a.size[l], a.size[l + 1], a.stride[l], a.pad[l], a.dil[l], in, slot_in, out,
                                                         slot_out, cnt, tid);
            else
                sp_conv_layer<CB, K>(a.W[l], a.B[l], Ci, Co, a.size[l], a.size[l + 1], a.stride[l], a.pad[l], a.dil[l], in, slot_in, out, slot_out, cnt, tid);
            __syncthreads();
        }
    }
}

// ---- the recurrence and the head --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDnThreads) void k_spatial_rnn(SpatialRnnArgs a) {
#define SP_RNN_DROPOUT 0
#include "susnet_spatial_rnn_body.h"
#undef SP_RNN_DROPOUT
}

// the training-mode form: dropout between the layers (the body's header says how)
__global__ __launch_bounds__(kDnThreads) void k_spatial_rnn_dropout(SpatialRnnArgs a, SpActDrop dr) {
#define SP_RNN_DROPOUT 1
#include "susnet_spatial_rnn_body.h"
#undef SP_RNN_DROPOUT
}

// susnet_rnn_dropout_mask: a thread per (layer, row, t, four units) writes the multipliers the dropout train step generates for itself
__global__ __launch_bounds__(256) void k_rnn_dropout_mask(SpDrop dr, int net, int layers, int64_t n, int T, int H, float *__restrict__ out) {
    const int HQ = (H + 3) >> 2;
    const int64_t total = (int64_t)(layers - 1) * n * T * HQ;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int q = (int)(e % HQ), t = (int)(e / HQ % T);
        const int64_t row = e / HQ / T % n;
        const int layer = (int)(e / HQ / T / n);
        float m[4];
        sp_drop4(dr, net, row, t, layer, q, m);
        float *dst = out + (((int64_t)layer * n + row) * T + t) * H;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * q + j < H) dst[4 * q + j] = m[j];
    }
}

// susnet_spatial_act_dropout_mask: the same thread shape over the acting rows, row r = (env r / agents, agent r % agents)
__global__ __launch_bounds__(256) void k_spatial_act_dropout_mask(SpActDrop dr, int layers, int64_t n, int T, int H, float *__restrict__ out) {
    const int HQ = (H + 3) >> 2;
    const int64_t total = (int64_t)(layers - 1) * n * T * HQ;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int q = (int)(e % HQ), t = (int)(e / HQ % T);
        const int64_t row = e / HQ / T % n, env = row / dr.agents;
        const int layer = (int)(e / HQ / T / n);
        float m[4];
        sp_drop4_at(dr.k0, dr.k1, dr.off_lo, dr.off_hi, dr.thr, dr.scale, dr.net, (int)(row - env * dr.agents), (uint64_t)(dr.row_base + env), t, layer,
                    q, m);
        float *dst = out + (((int64_t)layer * n + row) * T + t) * H;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * q + j < H) dst[4 * q + j] = m[j];
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
size_t spatial_conv_lds(SpatialConvArgs &a) {
    int s0 = a.C * a.size[0] * a.size[0], s1 = 0; // buffer 0: the input and what layers 1, 3 write; buffer 1: layers 0, 2; the last layer writes rnn_in
    for (int l = 0; l + 1 < a.n_conv; l++) {
        const int o = a.co[l] * a.size[l + 1] * a.size[l + 1];
        int &s = (l & 1) ? s0 : s1;
        s = o > s ? o : s;
    }
    a.slot0 = s0;
    a.slot1 = s1;
    const size_t per_image = (size_t)(s0 + s1) * sizeof(float);
    size_t g = kSpLdsGroup / per_image;
    g = g < 1 ? 1 : (g > (size_t)kSpGroup ? (size_t)kSpGroup : g);
    a.G = (int)g;
    return g * per_image;
}

size_t spatial_rnn_lds(SpatialRnnArgs &a) {
    int w = a.H;
    for (int l = 1; l + 1 < a.n_dims; l++) w = a.d[l] > w ? a.d[l] : w;
    a.buf = w * kDnRows;
    return (size_t)(a.L + 1) * a.buf * sizeof(float);
}

size_t spatial_rnn_dropout_lds(SpatialRnnArgs &a) {
    const size_t plain = spatial_rnn_lds(a);
    return plain + (size_t)(a.L > 2 ? 2 : 1) * a.buf * sizeof(float);
}

template <int CB, int K>
static hipError_t sp_conv_launch(const SpatialConvArgs &a, size_t lds, hipStream_t st) {
    if (lds > kSpLdsGroup) { // (one image alone is larger than the grouping target)
        static LdsOptIn opted;
        if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_spatial_conv<CB, K>), (int)kSpLdsBudget, opted)) return e;
    }
    const int64_t groups = (a.n * a.T + a.G - 1) / a.G;
    hipLaunchKernelGGL((k_spatial_conv<CB, K>), dim3((unsigned)(groups < kSpConvGrid ? groups : kSpConvGrid)), dim3(kSpThreads), lds, st, a);
    return hipGetLastError();
}
template <int K>
static hipError_t sp_conv_launch_k(const SpatialConvArgs &a, size_t lds, hipStream_t st) {
    int widest = 0;
    for (int l = 0; l < a.n_conv; l++) widest = a.co[l] > widest ? a.co[l] : widest;
    if (widest <= 4) return sp_conv_launch<4, K>(a, lds, st);
    if (widest <= 8) return sp_conv_launch<8, K>(a, lds, st);
    if (widest <= 16) return sp_conv_launch<16, K>(a, lds, st);
    return sp_conv_launch<32, K>(a, lds, st);
}

hipError_t spatial_conv_launch(SpatialConvArgs a, hipStream_t st) {
    const size_t lds = spatial_conv_lds(a);
    switch (a.k) {
    case 1: return sp_conv_launch_k<1>(a, lds, st);
    case 3: return sp_conv_launch_k<3>(a, lds, st);
    default: return sp_conv_launch_k<5>(a, lds, st);
    }
}

hipError_t spatial_rnn_launch(SpatialRnnArgs a, hipStream_t st) {
    const size_t lds = spatial_rnn_lds(a);
    if (lds > kDnLdsNoOptIn) {
        static LdsOptIn opted;
        if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_spatial_rnn), (int)kSpLdsBudget, opted)) return e;
    }
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    hipLaunchKernelGGL(k_spatial_rnn, dim3((unsigned)(tiles < kDnMaxGrid ? tiles : kDnMaxGrid)), dim3(kDnThreads), lds, st, a);
    return hipGetLastError();
}

hipError_t spatial_rnn_dropout_launch(SpatialRnnArgs a, const SpActDrop &d, hipStream_t st) {
    const size_t lds = spatial_rnn_dropout_lds(a);
    if (lds > kDnLdsNoOptIn) {
        static LdsOptIn opted;
        if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_spatial_rnn_dropout), (int)kSpLdsBudget, opted)) return e;
    }
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    hipLaunchKernelGGL(k_spatial_rnn_dropout, dim3((unsigned)(tiles < kDnMaxGrid ? tiles : kDnMaxGrid)), dim3(kDnThreads), lds, st, a, d);
    return hipGetLastError();
}

hipError_t rnn_dropout_mask_launch(const SpDrop &d, int net, int layers, int64_t n, int T, int H, float *out, hipStream_t st) {
    const int64_t total = (int64_t)(layers - 1) * n * T * ((H + 3) >> 2), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_rnn_dropout_mask, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, d, net, layers, n, T, H, out);
    return hipGetLastError();
}

hipError_t act_dropout_mask_launch(const SpActDrop &d, int layers, int64_t n, int T, int H, float *out, hipStream_t st) {
    const int64_t total = (int64_t)(layers - 1) * n * T * ((H + 3) >> 2), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_spatial_act_dropout_mask, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, d, layers, n, T, H, out);
    return hipGetLastError();
}

} // namespace susnet
