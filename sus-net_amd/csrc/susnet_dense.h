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

// the launch (inst_qnet_dense.hip); `a` validated by the caller
hipError_t qnet_dense_launch(DenseArgs a, hipStream_t st);
// dynamic LDS bytes of a layer stack, and buf1
size_t qnet_dense_lds(DenseArgs &a);

} // namespace susnet
