// susnet_mlp_train.h -- susnet_mlp_train_step: the DQN learner's train step (DQNTeamTrainer.train_step, src/train.py:50-149; susnet_train.h
// has the reference notes) for ANY served MLP stack on caller-supplied feature rows: 1 .. 7 Linear layers, F up to SUSNET_MLP_MAX_F, hidden
// widths up to 256, up to 32 outputs -- the layer stacks susnet_mlp_forward serves (susnet_dense.h).  The kernels: inst_mlp_train.hip.
//
// Per train step, on one stream, no host synchronisation, no atomics:
//   k_mlp_train_select  ONE workgroup: zeroes the gradient accumulators and the two losses and splits the n batch rows into a stable list per
//                       (agent, team) with its count -- as k_train_select, but the lists hold BATCH POSITIONS s (they index feat / next_feat);
//                       the ring row of a position is clamp(indices[s]).
//   per (agent, enabled team) update, two launches:
//   k_mlp_train_grad    a workgroup walks tiles of 32 of the list's rows.  Target network on next_feat (max over actions -> y, y = r on done
//                       rows), online network on feat, then 2 (Q - y) / count back through the stack; every matrix product on
//                       v_mfma_f32_32x32x2_f32 through susnet_train_core.h's tr_mfma / tr_forward_layer / tr_backward_layer on stride-33 transposed
//                       LDS tiles.  What differs from k_train_grad, because the stack is not known at compile time:
//                         - LDS holds two activation and two dZ buffers of 256 units (135 KB) whatever the stack; the input rows are never
//                           resident (layer 1 and its weight gradient read them from global memory), and the hidden pre-activations the backward
//                           pass needs go to the workgroup's own slice of the workspace, each thread reading back exactly the words it wrote;
//                         - the weight-gradient tiles do not stay in registers: each is one accumulator chain over the tile's 32 rows, added
//                           into the workgroup's own partial by read-modify-write (the first tile of a workgroup stores), one writer per word
//                           -- the same lane of the same wave on every tile; biases likewise, slopes and the loss in registers;
//                         - a workgroup without a tile zero-fills its partial; nothing at all runs for an empty list;
//                         - the layer loops are unrolled over the 7 possible layers with guards (the stack travels as a kernel argument).
//   k_train_adam        susnet_train.h's, as it is (susnet_capi_train.hip launches it): sums the partials in workgroup order, accumulates, Adam.
// Grid: G = min(kMtMaxGrid, tiles of n, kMtMaxPartialBytes / (4 Pp)) workgroups, at least 1: the partials stay at or below 64 MiB.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/susnet.h"

namespace susnet {

constexpr int kMtMaxLayers = 7, kMtMaxHidden = 256, kMtMaxOut = 32;
constexpr int kMtMaxGrid = 256;                         // workgroups of k_mlp_train_grad (one per CU)
constexpr uint64_t kMtMaxPartialBytes = 64ull << 20;    // all workgroups' partials together

// one team's stack in MLP.parameters() order: W0, b0, a0, W1, b1, a1, ..., W_last, b_last (float offsets into the flat parameter buffer)
struct MlpTrainNet {
    int32_t nl;     // Linear layers, 1 .. 7
    int32_t d[8];   // [F, h.., n_out]
    int32_t oW[7], oB[7], oA[6];
    int32_t zo[6];  // float offset of hidden layer l's saved pre-activations ([unit][32]) in a workgroup's slice
    int32_t P;      // parameters
    int32_t Pp;     // partial stride: P + 1 (the loss sum), rounded up to 4
    int32_t Z;      // floats of one workgroup's pre-activation slice
};

struct MlpTrainBatch {
    const float *feat, *next_feat; // [n][F]
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    const int16_t *imposters;
    const int64_t *idx;
    int64_t max_size, n;
    int32_t A, n_imp;
};

// the launches (inst_mlp_train.hip); arguments validated by the caller
hipError_t mlp_train_select_launch(const MlpTrainBatch &b, int32_t *lists, int32_t *counts, float *gacc0, int P0, float *gacc1, int P1, float *losses,
                                   hipStream_t st);
hipError_t mlp_train_grad_launch(const MlpTrainBatch &b, const MlpTrainNet &net, const float *prm, const float *tgt, const int32_t *lists,
                                 const int32_t *counts, int agent, int team, float gamma, float *partial, float *zsave, float *step, int G, hipStream_t st);

} // namespace susnet
