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
//
// A sweep (susnet_mlp_train_sweep): K learners of one shape in the launches of one, the learner is blockIdx.y.  k_mlp_train_sweep_select
// calls the same tr_select and k_mlp_train_sweep_grad includes the same body text (susnet_mlp_train_grad_body.h) as the single learner's
// kernels, so workgroup (g, k) does what workgroup g of learner k's own call does -- the same tiles g, g + G, .., the same partial slot
// and pre-activation slice, the same read-modify-write order -- and a learner's results are bitwise those of susnet_mlp_train_step.  A
// learner whose (agent, team) list is empty returns at once, whatever the others do, and its step count stays.  What the learners agree
// on travels once (the team's MlpTrainNet, n, A, n_imp; G is the grid); what differs is a per-learner record in a table passed BY VALUE
// as a kernel argument (no device table, no host copy: the call stays capturable).  The reduce + Adam launch is susnet_train.h's
// k_train_sweep_adam as it is: it reads P and Pp of its net argument only.  Learners never touch one another's memory.
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

// ---- the sweep's tables: one entry per learner, passed by value ----
constexpr int kMtSweepMaxLearners = SUSNET_MLP_SWEEP_MAX_LEARNERS;
struct MlpSweepSelLearner { // k_mlp_train_sweep_select
    const int16_t *imposters;
    const int64_t *idx;
    int64_t max_size;
    int32_t *lists, *counts;
    float *gacc0, *gacc1, *losses;
};
struct MlpSweepSelTable {
    MlpSweepSelLearner l[kMtSweepMaxLearners];
};
struct MlpSweepLearner { // one team of one learner: k_mlp_train_sweep_grad -- the MlpTrainBatch fields that differ, then the kernel's own arguments
    const float *feat, *next_feat;
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    const int16_t *imposters;
    const int64_t *idx;
    int64_t max_size;
    const float *prm, *tgt;
    const int32_t *lists, *counts;
    float *partial, *zsave, *step;
    float gamma;
    int32_t pad_;
};
struct MlpSweepTable {
    MlpSweepLearner l[kMtSweepMaxLearners];
};
static_assert(sizeof(MlpSweepTable) + sizeof(MlpTrainNet) + 64 <= 4096 && sizeof(MlpSweepSelTable) + 64 <= 4096, "the tables are kernel arguments: 4 KB");

// the launches (inst_mlp_train.hip); arguments validated by the caller
hipError_t mlp_train_select_launch(const MlpTrainBatch &b, int32_t *lists, int32_t *counts, float *gacc0, int P0, float *gacc1, int P1, float *losses,
                                   hipStream_t st);
hipError_t mlp_train_grad_launch(const MlpTrainBatch &b, const MlpTrainNet &net, const float *prm, const float *tgt, const int32_t *lists,
                                 const int32_t *counts, int agent, int team, float gamma, float *partial, float *zsave, float *step, int G, hipStream_t st);
// the sweep forms: grid (1, K) and (G, K); n, A, n_imp and `net` are the learners' common ones
hipError_t mlp_train_sweep_select_launch(const MlpSweepSelTable &tab, int K, int64_t n, int A, int n_imp, int P0, int P1, hipStream_t st);
hipError_t mlp_train_sweep_grad_launch(const MlpSweepTable &tab, int K, const MlpTrainNet &net, int64_t n, int A, int n_imp, int agent, int team, int G,
                                       hipStream_t st);

} // namespace susnet
