// the dense Q-network kernel (susnet_dense.h: susnet_mlp_forward) -- a translation unit of its own, default scheduling like the other
// Q-network units
#include "susnet_dense.h"

#include "susnet_host.h" // lds_opt_in

namespace susnet {

typedef float dn_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float dn_prelu(float z, float a) { return z > 0.0f ? z : a * z; } // torch.prelu
// register r of a 32 x 32 result tile is row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32
__device__ __forceinline__ int dn_row(int r, int lane) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }
// LDS float index of (unit u, row s of the 64-row tile): odd units keep their two 32-row halves swapped
__device__ __forceinline__ int dn_lds(int u, int s) { return u * kDnRows + (s ^ ((u & 1) << 5)); }

// the operands of chunk c (k = 32 c .. 32 c + 31) of one block: lane (i, h) feeds k = 32 c + 2 s + h for step s.  Addresses are clamped into
// the row (k <= dk - 1); what lies past the edge becomes a zero operand.
template <bool BGLOBAL>
__device__ __forceinline__ void dn_load(const float *__restrict__ wrow, const float *__restrict__ xrow, bool svalid, int dk, int c, int h, float (&a)[16],
                                        float (&b)[16]) {
#pragma unroll
    for (int s = 0; s < 16; s++) {
        const int p = 32 * c + 2 * s + h, pc = p < dk ? p : dk - 1;
        const float av = wrow[pc];
        a[s] = p < dk ? av : 0.0f;
        if constexpr (BGLOBAL) {
            const float bv = xrow[pc];
            b[s] = (p < dk && svalid) ? bv : 0.0f;
        }
    }
}

// one block: units n0 .. n0 + 31 of a layer for rows st * 32 .. st * 32 + 31 of the tile.  acc starts as the bias; one chain over k, ascending.
template <bool BGLOBAL>
__device__ __forceinline__ dn_f32x16 dn_block(const float *__restrict__ W, const float *__restrict__ bias, int dk, int dn, int n0, int st,
                                              const float *__restrict__ xrow, bool svalid, const float *zin, int lane) {
    const int i = lane & 31, h = lane >> 5;
    dn_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int u = n0 + dn_row(r, lane);
        const float bv = bias[u < dn ? u : dn - 1];
        acc[r] = u < dn ? bv : 0.0f;
    }
    const int ur = n0 + i < dn ? n0 + i : dn - 1; // (a unit past the width: its operands are zeroed below, its results never stored)
    const bool uvalid = n0 + i < dn;
    const float *wrow = W + (size_t)ur * dk;
    const int nch = (dk + 31) >> 5;
    float a0[16], b0[16];
    dn_load<BGLOBAL>(wrow, xrow, svalid, dk, 0, h, a0, b0);
    for (int c = 0; c < nch; c++) {
        float a1[16], b1[16];
#pragma unroll
        for (int s = 0; s < 16; s++) a1[s] = b1[s] = 0.0f;
        if (c + 1 < nch) dn_load<BGLOBAL>(wrow, xrow, svalid, dk, c + 1, h, a1, b1); // (wave-uniform)
        if constexpr (!BGLOBAL) {
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const int p = 32 * c + 2 * s + h, pc = p < dk ? p : dk - 1;
                const float bv = zin[dn_lds(pc, st * 32 + i)];
                b0[s] = p < dk ? bv : 0.0f;
            }
        }
#pragma unroll
        for (int s = 0; s < 16; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(uvalid ? a0[s] : 0.0f, b0[s], acc, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 16; s++) {
            a0[s] = a1[s];
            b0[s] = b1[s];
        }
    }
    return acc;
}

__global__ __launch_bounds__(kDnThreads) void k_qnet_dense(DenseArgs a) {
    extern __shared__ float dn_smem[];
    const int t = threadIdx.x, lane = t & 63, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nl = a.n_dims - 1;
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kDnRows;
        for (int l = 0; l < nl; l++) {
            const int dk = a.d[l], dn = a.d[l + 1];
            const float *W = a.W[l], *bias = a.B[l];
            const bool last = l == nl - 1;
            const float slope = last ? 1.0f : a.A[l][0];
            const float *zin = dn_smem + ((l & 1) ? 0 : a.buf1); // what layer l - 1 wrote
            float *zout = dn_smem + ((l & 1) ? a.buf1 : 0);
            const int items = ((dn + 31) >> 5) * 2;
            for (int it = wave; it < items; it += kDnWaves) {
                const int n0 = (it >> 1) * 32, st = it & 1;
                const int64_t s = base + st * 32 + i;
                const bool svalid = s < a.n;
                dn_f32x16 acc;
                if (l == 0) {
                    const float *xrow = a.rows + (size_t)(svalid ? s : a.n - 1) * dk;
                    acc = dn_block<true>(W, bias, dk, dn, n0, st, xrow, svalid, nullptr, lane);
                } else {
                    acc = dn_block<false>(W, bias, dk, dn, n0, st, nullptr, svalid, zin, lane);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int u = n0 + dn_row(r, lane);
                    if (u < dn) {
                        if (last) {
                            if (svalid) a.q[(size_t)s * dn + u] = acc[r];
                        } else {
                            zout[dn_lds(u, st * 32 + i)] = dn_prelu(acc[r], slope);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

size_t qnet_dense_lds(DenseArgs &a) {
    int w0 = 0, w1 = 0; // widest output of the layers that write buffer 0 (1st, 3rd, ..) / buffer 1; the last layer writes q_out
    for (int l = 0; l + 2 < a.n_dims; l++) {
        int &w = (l & 1) ? w1 : w0;
        w = a.d[l + 1] > w ? a.d[l + 1] : w;
    }
    a.buf1 = w0 * kDnRows;
    return (size_t)(w0 + w1) * kDnRows * sizeof(float);
}

hipError_t qnet_dense_launch(DenseArgs a, hipStream_t st) {
    const size_t lds = qnet_dense_lds(a);
    if (lds > kDnLdsNoOptIn) { // the opt-in to a large dynamic LDS block: once per device, off the per-tick path after that
        static LdsOptIn opted;
        if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_qnet_dense), 2 * kDnMaxHidden * kDnRows * 4, opted)) return e;
    }
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    hipLaunchKernelGGL(k_qnet_dense, dim3((unsigned)(tiles < kDnMaxGrid ? tiles : kDnMaxGrid)), dim3(kDnThreads), lds, st, a);
    return hipGetLastError();
}

} // namespace susnet
