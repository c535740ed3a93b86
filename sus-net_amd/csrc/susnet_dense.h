// susnet_dense.h -- susnet_mlp_forward: the reference MLP (src/models/dqn.py:72-108, make_mlp 322-329: Linear + nn.PReLU() with one slope
// per layer, no activation after the last Linear) of ANY served layer stack on caller-supplied feature rows, as one kernel.
//
// Unlike the compiled-in family (susnet_qnet.h: a packed image for one feature layout, the feature row built from the state words), this
// kernel reads the weights where torch keeps them ([out][in] row-major, 4-byte aligned only: dword loads throughout) and the feature rows
// from memory; there is no host step, so an in-place optimizer step is seen by the next launch.
//
//   k_qnet_dense   a workgroup of 8 waves walks tiles of 64 rows (grid-stride).  Per layer the work items are (32 output units) x (32 rows)
//                  blocks, dealt round-robin to the waves; a block is ONE accumulator tile of v_mfma_f32_32x32x2_f32 that starts as the
//                  bias and runs over k in ascending order, 32 k per chunk: the chunk's weight operands (and, for layer 1, the input
//                  operands: the input row is never resident in LDS, so F is not bounded by it) are loaded one chunk ahead of the matrix
//                  instructions.  Hidden activations live in LDS only, transposed [unit][row] with 64 rows per unit and the two halves of
//                  odd units swapped (the two k of one matrix instruction then read disjoint banks), PReLU applied once, at the write.
//                  Ragged edges -- rows past n, units past a layer's width, k past its input width -- are ZERO operands made in
//                  registers: every address is clamped into its array before the load, nothing is read or written past an array's end.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/susnet.h"

namespace susnet {

constexpr int kDnThreads = 512, kDnWaves = kDnThreads / 64, kDnRows = SUSNET_MLP_ROW_TILE, kDnMaxGrid = SUSNET_MLP_MAX_GRID;
constexpr int kDnMaxHidden = 256, kDnMaxOut = 32;
constexpr size_t kDnLdsNoOptIn = 48 * 1024; // a dynamic LDS block up to this size launches without the opt-in (lds_opt_in, susnet_host.h)
static_assert(kDnRows == 64, "the LDS layout below is 64 rows per unit");

struct DenseArgs { // by value: the kernel's arguments
    int32_t n_dims;
    int32_t d[8];
    const float *W[7], *B[7], *A[6];
    const float *rows;
    int64_t n;
    float *q;
    int32_t buf1; // float offset of the second activation buffer (layers 2, 4, 6 write it; layers 1, 3, 5 write offset 0)
};

// ---- device code of a block, shared with the recurrent kernel of susnet_spatial.h (inst_qnet_spatial.hip) ----
#ifdef __HIPCC__
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

// the accumulator tile of units n0 .. n0 + 31 at its start: the bias (and, for a recurrent layer, a second bias added to it in float32)
__device__ __forceinline__ dn_f32x16 dn_bias(const float *__restrict__ bias, const float *__restrict__ bias2, int dn, int n0, int lane) {
    dn_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int u = n0 + dn_row(r, lane), uc = u < dn ? u : dn - 1;
        float bv = bias[uc];
        if (bias2) bv += bias2[uc];
        acc[r] = u < dn ? bv : 0.0f;
    }
    return acc;
}

// one weight matrix W [dn][dk] folded into a block's accumulator: units n0 .. n0 + 31 of a layer for rows st * 32 .. st * 32 + 31 of the
// tile, one chain over k, ascending.  (A recurrent layer calls this twice on the same accumulator: W_ih over x_t, then W_hh over h_{t-1}.)
template <bool BGLOBAL>
__device__ __forceinline__ dn_f32x16 dn_chain(dn_f32x16 acc, const float *__restrict__ W, int dk, int dn, int n0, int st,
                                              const float *__restrict__ xrow, bool svalid, const float *zin, int lane) {
    const int i = lane & 31, h = lane >> 5;
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

// one block of a Linear layer: acc starts as the bias; one chain over k, ascending.
template <bool BGLOBAL>
__device__ __forceinline__ dn_f32x16 dn_block(const float *__restrict__ W, const float *__restrict__ bias, int dk, int dn, int n0, int st,
                                              const float *__restrict__ xrow, bool svalid, const float *zin, int lane) {
    return dn_chain<BGLOBAL>(dn_bias(bias, nullptr, dn, n0, lane), W, dk, dn, n0, st, xrow, svalid, zin, lane);
}

#endif

// the launch (inst_qnet_dense.hip); `a` validated by the caller
hipError_t qnet_dense_launch(DenseArgs a, hipStream_t st);
// dynamic LDS bytes of a layer stack, and buf1
size_t qnet_dense_lds(DenseArgs &a);

} // namespace susnet
