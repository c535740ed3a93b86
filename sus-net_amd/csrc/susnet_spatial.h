// susnet_spatial.h -- susnet_spatial_forward: the eval-mode forward of the reference SpatialDQN (src/models/dqn.py:205-301: a Conv2d + ReLU
// stack per window step, 141-181; the flattened result and that step's non-spatial features through nn.RNN(tanh), 184-202, 294-296; the
// PReLU head on the last layer's last hidden state, 298-299) in float32, as two kernels.  Parameters are read where torch keeps them
// (4-byte aligned only, no packed image, no host step: the next launch sees an in-place optimizer step), as susnet_mlp_forward reads them.
//
//   k_spatial_conv  vector ALU.  A workgroup of 256 lanes walks groups of G images (an image = one window step of one (env, agent) row;
//                   grid-stride).  The group's images [C][N][N] are copied into LDS; a layer reads one LDS buffer and writes the other,
//                   the last layer writes the RNN input row in global memory ([C_out][H][W] order, torch's flatten) and the step's
//                   non-spatial features are copied behind it.  A work item is one output pixel of one image -- the images lie back to
//                   back over the lanes -- and keeps ALL output channels of its pixel in registers (template CB = 4 / 8 / 16 / 32: the
//                   smallest that holds the layer's width), so an input tap is read from LDS once per layer.  Every output is one fmaf
//                   chain that starts as the bias and runs over (c_in, ky, kx) in ascending order; the weights come through wave-uniform
//                   loads (the index does not depend on the lane) and are the FMA's scalar operand; a padding tap is a zero made in a
//                   register (its LDS address is clamped into the image), never an out-of-bounds read.  K = 1 / 3 / 5 is a template
//                   parameter: the taps' offsets and bounds are then loop-invariant over c_in.  The kernel is compiled per (CB, K), CB being
//                   the width class of the stack's widest layer (a layer of at most half of it runs the next narrower form), so a
//                   narrow stack does not carry a wide one's registers.
//   k_spatial_rnn   v_mfma_f32_32x32x2_f32, the dense kernel's tile machinery (susnet_dense.h: dn_bias / dn_chain) with a second weight
//                   matrix.  A workgroup of 8 waves walks tiles of 64 rows; for t = 0 .. T - 1 and layer l = 0 .. L - 1 a block's
//                   accumulator starts as b_ih + b_hh, runs over W_ih (k ascending; layer 0 reads x_t from rnn_in in global memory, so R
//                   is not bounded by LDS) and then, for t > 0, over W_hh on h_l[t-1] (h = 0 at t = 0: nothing is added), and tanh is
//                   applied at the write into LDS.  Hidden states live in LDS only, in L + 1 buffers of the dense kernel's [unit][64 rows]
//                   layout that rotate: step c = t L + l writes buffer c mod (L + 1), h_{l-1}[t] is in buffer c - 1 and h_l[t-1] in
//                   buffer c + 1 (mod L + 1).  The head runs on the last buffer as the dense kernel's layers do.
//   k_spatial_rnn_dropout   the same text (susnet_spatial_rnn_body.h, included twice) in nn.RNN's TRAINING mode, for
//                   susnet_spatial_forward_dropout: the output of every layer below the top one also goes, multiplied by its dropout mask
//                   (susnet_dropout.h: sp_drop4_at, one Philox block per four consecutive units of a row -- registers 4 q .. 4 q + 3 of the
//                   accumulator), into a buffer D behind the rotation, which the layer above reads in place of h_{l-1}[t]; the layer's own
//                   recurrence and the head read the undropped values.  Layer l writes D[l & 1] and reads D[(l - 1) & 1]: one buffer at
//                   L = 2, two from L = 3 on (a step's waves read and write D between the same two barriers).
//   tanh            sp_tanh below: e = expm1f(-2 |x|), tanh = copysign(-e / (e + 2), x): no cancellation near 0 (tanh(+-0) = +-0 exactly),
//                   and for |x| >= 16 the result is set to +-1 (expm1f has long returned -1 exactly there: e^-32 < 2^-25).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/susnet.h"
#include "susnet_dense.h"
#include "susnet_dropout.h"

namespace susnet {

constexpr int kSpThreads = 256, kSpMaxConv = SUSNET_SPATIAL_MAX_CONV, kSpGroup = SUSNET_SPATIAL_CONV_GROUP, kSpConvGrid = SUSNET_SPATIAL_CONV_MAX_GRID;
constexpr int kSpMaxRnn = SUSNET_SPATIAL_MAX_RNN_LAYERS;
constexpr size_t kSpLdsBudget = 160 * 1024;  // a workgroup's LDS on gfx950
constexpr size_t kSpLdsGroup = 48 * 1024;    // images are grouped up to this much LDS (no opt-in below it, three workgroups per CU)

struct SpatialConvArgs { // by value: the kernel's arguments
    int32_t T, C, n_conv, k, Fn, agents, R;
    int32_t size[kSpMaxConv + 1];                                   // size[0] = N, size[l + 1] = layer l's output size
    int32_t co[kSpMaxConv], stride[kSpMaxConv], pad[kSpMaxConv], dil[kSpMaxConv];
    const float *W[kSpMaxConv], *B[kSpMaxConv];
    const float *spatial, *non_spatial;
    int64_t sp_stride[3], ns_stride[3]; // floats: per env, per agent, per timestep
    int64_t n;
    float *rnn_in;
    int32_t G, slot0, slot1; // images per group; floats per image in LDS buffer 0 (the input, layers 1 and 3) and 1 (layers 0 and 2)
};

struct SpatialRnnArgs {
    int32_t T, R, L, H;
    const float *w_ih[kSpMaxRnn], *w_hh[kSpMaxRnn], *b_ih[kSpMaxRnn], *b_hh[kSpMaxRnn];
    int32_t n_dims;
    int32_t d[8];
    const float *W[7], *B[7], *A[6];
    const float *rnn_in;
    int64_t n;
    float *q;
    int32_t buf; // floats per hidden-state buffer: 64 rows x the widest of H and the head's hidden layers
};

#ifdef __HIPCC__
// tanh as the forward (inst_qnet_spatial.hip) and the learner (inst_spatial_train.hip) compute it: exactly 0 at 0, exactly +-1 from |x| = 16
__device__ __forceinline__ float sp_tanh(float x) {
    const float ax = fabsf(x);
    const float e = expm1f(-2.0f * ax); // in (-1, 0]: tanh |x| = (1 - e^{-2|x|}) / (1 + e^{-2|x|}) = -e / (e + 2), no cancellation near 0
    const float t = ax >= 16.0f ? 1.0f : -e / (e + 2.0f);
    return copysignf(t, x);
}
#endif

// LDS bytes of a call's two kernels; they also fill in G / slot0 / slot1 and buf
size_t spatial_conv_lds(SpatialConvArgs &a);
size_t spatial_rnn_lds(SpatialRnnArgs &a);
size_t spatial_rnn_dropout_lds(SpatialRnnArgs &a); // (L + 2) buffers at L = 2, (L + 3) from L = 3 on
// the launches (inst_qnet_spatial.hip); arguments validated by the caller, LDS within kSpLdsBudget
hipError_t spatial_conv_launch(SpatialConvArgs a, hipStream_t st);
hipError_t spatial_rnn_launch(SpatialRnnArgs a, hipStream_t st);
hipError_t spatial_rnn_dropout_launch(SpatialRnnArgs a, const SpActDrop &d, hipStream_t st); // a.L >= 2, d.thr != 0

} // namespace susnet
