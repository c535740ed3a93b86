// susnet_train.h -- the DQN learner's train step (DQNTeamTrainer.train_step) on the device: TD targets, MSE gradient, Adam, re-pack.
//
// Reference behaviour (paths relative to the reference repo root):
//   DQNTeamTrainer.train_step        src/train.py:50-149   per agent, imposter team then crew team: masked rows, online Q, target max,
//                                                          MSE, backward (gradients ACCUMULATE: zero_grad once per call, 64-67), Adam step
//   torch.optim.Adam (defaults)      src/train.py:24-38    betas (0.9, 0.999), eps 1e-8, single-tensor update order
//   ReplayBuffer.sample              src/replay_memory.py:75-94  (the indices; the ring tensors are read in place here)
//   MLP / make_mlp                   src/models/dqn.py:72-88, 322-329
//
// Per train step (all on one stream, no host synchronisation, every decision on the device):
//   k_train_select   ONE workgroup: zeroes the gradient accumulators and the two losses, and splits the N sampled ring rows into a
//                    stable list per (agent, team) -- imposter rows = imposters[row, 0] == agent -- with its count.
//   per (agent, team) update, two launches:
//   k_train_grad     a workgroup walks tiles of 32 of the team's rows: builds the FlatFeaturizer rows in LDS (susnet_flat.h's row
//                    decoding), runs the target network (max over actions -> y, y = r on done rows), the online network (pre-activations
//                    kept in LDS), and back-propagates 2 (Q - y) / n through the five Linear layers and the four PReLUs.  Every matrix
//                    product -- forward, the transposed weights of backward, the weight gradients -- runs on v_mfma_f32_32x32x2_f32 with
//                    activations stored transposed ([unit][sample], row stride 33 floats: no bank conflict for either operand order).
//                    The weight-gradient tiles of the whole network stay in each wave's accumulators across the workgroup's tiles and are
//                    written once, with the bias / slope / loss sums, as the workgroup's partial: no atomics, one writer per word.
//   k_train_adam     thread per parameter: sums the partials in workgroup order (bitwise reproducible), adds them to the step's gradient
//                    accumulator, applies Adam on the torch-layout parameters; does nothing when the team's count is 0.
//   per team and step, one launch:
//   k_train_pack     the team's packed image (susnet_qnet_pack's layout, susnet_capi_nets.hip) from the updated parameters, element for element
//                    the host's arithmetic (tail rows summed in its order): bitwise what the host packer makes.
//
// A sweep (susnet_dqn_train_sweep; the notebooks' loops over run_experiment(**config), notebooks/experiment_1v1.ipynb and
// experiment_mlp.ipynb) trains K learners of one shape in the SAME launches: k_train_sweep_select / _grad / _adam / _pack take a table of
// per-learner arguments by value (TrainTable, TrainSelTable) and the learner is blockIdx.y.  Each kernel body is ONE __device__ function
// (tr_select / tr_grad / tr_adam / tr_pack) that both forms call, the single-learner kernel with its own arguments and the sweep kernel
// with table.l[blockIdx.y]: workgroup (g, k) of a sweep does exactly what workgroup g of learner k's own call does -- same tiles, same
// partial layout, same order of every sum -- so a learner's results are bitwise those of susnet_dqn_train_step.  Learners never touch
// one another's memory: no waits between workgroups, no atomics.
// What the dense learner shares (tr_mfma and the layer functions, tr_select, tr_block_sum, tr_adam, the host-side layouts) is
// susnet_train_core.h; the structures and every kernel are here -- k_train_adam too, which susnet_capi_train.hip launches for both learners.
#pragma once

#include "susnet_flat.h"
#include "susnet_train_core.h"

namespace susnet {

constexpr int kTrMaxF = 96;        // input width cap (the compiled-in layouts: 36, 4, 88)
constexpr int kTrMaxTiles = 9;     // weight-gradient tiles per wave: (3 x 8 + 8 x 4 + 4 x 2 + 2 + 1 = 67) / 8 waves, rounded up
constexpr int kTrMaxGrid = 256;    // workgroups of k_train_grad (one per CU)
constexpr int kTrMaxLearners = SUSNET_DQN_MAX_LEARNERS; // learners of one sweep call (the tables travel as kernel arguments)

// one team's network in torch's parameter order (MLP.parameters(): model.0.weight, model.0.bias, model.1.weight (PReLU), model.2.weight ...)
struct TrainNet {
    int32_t d[6];
    int32_t oW[5], oB[5], oA[4];
    int32_t P;    // parameters
    int32_t Pp;   // partial stride: P + 1 (the loss sum), rounded up to 4
};

struct TrainRing {
    const float *states, *next_states;
    const int64_t *actions;
    const float *rewards;
    const uint8_t *dones;
    const int16_t *imposters;
    int64_t max_size;
    int32_t S, A, n_imp;
};

// ---- the sweep's tables: one entry per learner, passed by value ----
struct TrainSelLearner { // k_train_sweep_select
    TrainRing ring;
    const int64_t *idx;
    int32_t *lists, *counts;
    float *gacc0, *gacc1, *losses;
};
struct TrainSelTable {
    TrainSelLearner l[kTrMaxLearners];
};
struct TrainLearner { // one team of one learner: k_train_sweep_grad / _adam / _pack
    TrainRing ring;
    float *prm;
    const float *tgt;
    float *m1, *m2, *step;
    const int32_t *lists, *counts;
    float *gacc, *partial, *losses, *packed;
    double lr, beta1, beta2, eps;
    float gamma;
    int32_t pad_;
};
struct TrainTable {
    TrainLearner l[kTrMaxLearners];
};
static_assert(sizeof(TrainTable) + sizeof(TrainNet) + 64 <= 4096 && sizeof(TrainSelTable) + 64 <= 4096, "the tables are kernel arguments: 4 KB");

// LDS (floats): activations transposed [unit][sample] with row stride kTrSP
constexpr int kTrOX = 0, kTrOZ1 = kTrOX + kTrMaxF * kTrSP, kTrOZ2 = kTrOZ1 + 256 * kTrSP, kTrOZ3 = kTrOZ2 + 128 * kTrSP,
              kTrOZ4 = kTrOZ3 + 64 * kTrSP, kTrOZ5 = kTrOZ4 + 32 * kTrSP, kTrODA = kTrOZ5 + 32 * kTrSP, kTrODB = kTrODA + 128 * kTrSP,
              kTrOY = kTrODB + 256 * kTrSP, kTrOAct = kTrOY + kTrTS, kTrORow = kTrOAct + kTrTS, kTrOMask = kTrORow + kTrTS,
              kTrOVal = kTrOMask + 3 * kTrTS, kTrLdsFloats = kTrOVal + 4 * kTrTS;
constexpr int kTrLdsBytes = kTrLdsFloats * 4;
static_assert(kTrLdsBytes <= 160 * 1024, "gfx950 LDS");

// ---- k_train_select: ONE workgroup of kTrThreads (per learner); the lists hold ring rows ----
__global__ __launch_bounds__(kTrThreads) void k_train_select(TrainRing ring, const int64_t *__restrict__ idx, int64_t N, int32_t *lists, int32_t *counts,
                                                             float *gacc0, int P0, float *gacc1, int P1, float *losses) {
    extern __shared__ int32_t tr_scan[];
    tr_select<false>(ring, idx, N, lists, counts, gacc0, P0, gacc1, P1, losses, tr_scan);
}
__global__ __launch_bounds__(kTrThreads) void k_train_sweep_select(TrainSelTable tab, int64_t N, int P0, int P1) {
    extern __shared__ int32_t tr_scan[];
    const TrainSelLearner &a = tab.l[blockIdx.y];
    tr_select<false>(a.ring, a.idx, N, a.lists, a.counts, a.gacc0, P0, a.gacc1, P1, a.losses, tr_scan);
}

// the tile's feature rows X[k][s] (k < F) from flattened states (base.py:234-235: positions, then alive flags)
template <class ROW>
__device__ __forceinline__ void tr_build_x(const float *__restrict__ rows, int S, const float *lds_f, float *lds, int nvalid, int t) {
    constexpr int A = ROW::A, F = ROW::F;
    const int32_t *rid = reinterpret_cast<const int32_t *>(lds_f + kTrORow);
    if constexpr (ROW::kDeadZero) {
        uint32_t *mask = reinterpret_cast<uint32_t *>(lds + kTrOMask);
        if (t < kTrTS) {
            ROW row;
            row.clear();
            if (t < nvalid) {
                const float *v = rows + (int64_t)rid[t] * S;
                uint32_t x[A], y[A], al[A];
                bool ok = true;
#pragma unroll
                for (int i = 0; i < A; i++) {
                    const int xi = (int)v[2 * i], yi = (int)v[2 * i + 1];
                    ok = ok && (unsigned)xi < (unsigned)ROW::N && (unsigned)yi < (unsigned)ROW::N;
                    x[i] = (uint32_t)xi & 15u;
                    y[i] = (uint32_t)yi & 15u;
                    al[i] = v[2 * A + i] != 0.0f ? 1u : 0u;
                }
                if (ok) row.build(x, y, al);
            }
#pragma unroll
            for (int w = 0; w < 3; w++) mask[w * kTrTS + t] = w < ROW::MW ? row.m[w] : 0u;
        }
        __syncthreads();
        for (int e = t; e < F * kTrTS; e += kTrThreads) {
            const int k = e / kTrTS, s = e % kTrTS;
            lds[kTrOX + k * kTrSP + s] = (float)((mask[(k >> 5) * kTrTS + s] >> (k & 31)) & 1u);
        }
    } else { // CoordRow: [x0, y0, x1, y1] as floats (component.py:384-403)
        for (int e = t; e < F * kTrTS; e += kTrThreads) {
            const int k = e / kTrTS, s = e % kTrTS;
            lds[kTrOX + k * kTrSP + s] = s < nvalid ? rows[(int64_t)rid[s] * S + k] : 0.0f;
        }
    }
    __syncthreads();
}

template <class ROW>
__device__ __forceinline__ void tr_forward(const TrainNet &net, const float *__restrict__ prm, float *lds, int wave, int lane) {
    const int *d = net.d;
    const int zo[6] = {kTrOX, kTrOZ1, kTrOZ2, kTrOZ3, kTrOZ4, kTrOZ5};
#pragma unroll
    for (int l = 0; l < 5; l++) {
        tr_forward_layer(prm + net.oW[l], prm + net.oB[l], d[l], d[l + 1], lds + zo[l], l > 0 ? prm[net.oA[l - 1]] : 1.0f, l == 0, lds + zo[l + 1], wave,
                         lane);
        __syncthreads();
    }
}

// ---- k_train_grad: one (agent, team) update's gradient partials; workgroup blockIdx.x of gridDim.x ----
template <class ROW>
__device__ __forceinline__ void tr_grad(const TrainRing &ring, const TrainNet &net, const float *__restrict__ prm, const float *__restrict__ tgt,
                                        const int32_t *__restrict__ lists, const int32_t *__restrict__ counts, int64_t N, int agent, int team, float gamma,
                                        float *__restrict__ partial, float *step, float *lds) {
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int count = counts[2 * agent + team];
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * N;
    if (blockIdx.x == 0 && t == 0 && count > 0) step[0] += 1.0f; // (k_train_adam reads it after this launch)
    const int *d = net.d;
    int tbase[6]; // first global tile id of each layer's weight gradient
    tbase[0] = 0;
    for (int l = 0; l < 5; l++) tbase[l + 1] = tbase[l] + ((d[l + 1] + 31) / 32) * ((d[l] + 31) / 32);
    int bbase[6];
    bbase[0] = 0;
    for (int l = 0; l < 5; l++) bbase[l + 1] = bbase[l] + d[l + 1];
    tr_f32x16 acc[kTrMaxTiles];
#pragma unroll
    for (int m = 0; m < kTrMaxTiles; m++) acc[m] = tr_f32x16{};
    float bacc = 0.0f, lacc = 0.0f, sacc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float inv_n = count > 0 ? 2.0f / (float)count : 0.0f; // mse_loss backward: 2 (x - y) / numel
    const int zo[6] = {kTrOX, kTrOZ1, kTrOZ2, kTrOZ3, kTrOZ4, kTrOZ5};
    const int n_out = d[5];
    for (int tile = blockIdx.x; tile * kTrTS < count; tile += gridDim.x) {
        const int base = tile * kTrTS, nvalid = count - base < kTrTS ? count - base : kTrTS;
        int32_t *rid = reinterpret_cast<int32_t *>(lds + kTrORow);
        int32_t *act = reinterpret_cast<int32_t *>(lds + kTrOAct);
        if (t < kTrTS) rid[t] = t < nvalid ? list[base + t] : 0;
        __syncthreads();
        // target network on the next states: y = r + gamma max_a Q'(s', a); y = r where done (train.py:121-134)
        tr_build_x<ROW>(ring.next_states, ring.S, lds, lds, nvalid, t);
        tr_forward<ROW>(net, tgt, lds, wave, lane);
        if (t < kTrTS) {
            float y = 0.0f;
            int a = 0;
            if (t < nvalid) {
                const int64_t r = rid[t];
                float m = lds[kTrOZ5 + t];
                for (int j = 1; j < n_out; j++) m = fmaxf(m, lds[kTrOZ5 + j * kTrSP + t]);
                const float rew = ring.rewards[r * ring.A + agent];
                y = ring.dones[r] ? rew : rew + gamma * m;
                a = (int)ring.actions[r * ring.A + agent];
                a = a < 0 ? 0 : (a >= n_out ? n_out - 1 : a);
            }
            lds[kTrOY + t] = y;
            act[t] = a;
        }
        __syncthreads();
        // online network on the states, pre-activations kept
        tr_build_x<ROW>(ring.states, ring.S, lds, lds, nvalid, t);
        tr_forward<ROW>(net, prm, lds, wave, lane);
        // dL/dQ into DB (rows n_out): 2 (Q - y) / n at the taken action, 0 elsewhere and on padding columns
        for (int e = t; e < n_out * kTrTS; e += kTrThreads) {
            const int j = e / kTrTS, s = e % kTrTS;
            float g = 0.0f;
            if (s < nvalid && j == act[s]) g = inv_n * (lds[kTrOZ5 + j * kTrSP + s] - lds[kTrOY + s]);
            lds[kTrODB + j * kTrSP + s] = g;
        }
        if (t < nvalid) {
            const float diff = lds[kTrOZ5 + act[t] * kTrSP + t] - lds[kTrOY + t];
            lacc += diff * diff;
        }
        __syncthreads();
        // backward, layer 5 .. 1: dz of layer l in DB (l = 4, 2, 0) or DA (l = 3, 1)
#pragma unroll
        for (int l = 4; l >= 0; l--) {
            float *dz = lds + ((l & 1) ? kTrODA : kTrODB);
            float *dh = lds + ((l & 1) ? kTrODB : kTrODA);
            const float *zin = lds + zo[l];
            const float slope_in = l > 0 ? prm[net.oA[l - 1]] : 1.0f;
            // weight gradient tiles of layer l: dW[n][k] += sum_s dz[n][s] h_in[k][s]
            const int KT = (d[l] + 31) / 32;
#pragma unroll
            for (int m = 0; m < kTrMaxTiles; m++) {
                const int g = m * kTrWaves + wave;
                if (g >= tbase[l] && g < tbase[l + 1]) {
                    const int n0 = ((g - tbase[l]) / KT) * 32, k0 = ((g - tbase[l]) % KT) * 32;
                    const int dn = d[l + 1], dk = d[l];
                    acc[m] = tr_mfma([&](int i, int p) { return n0 + i < dn ? dz[(n0 + i) * kTrSP + p] : 0.0f; },
                                     [&](int p, int j) {
                                         if (k0 + j >= dk) return 0.0f;
                                         const float z = zin[(k0 + j) * kTrSP + p];
                                         return l == 0 ? z : tr_prelu(z, slope_in);
                                     },
                                     kTrTS, acc[m], lane);
                }
            }
            if (t >= bbase[l] && t < bbase[l + 1]) { // bias gradient
                const int n = t - bbase[l];
                float s = 0.0f;
                for (int j = 0; j < kTrTS; j++) s += dz[n * kTrSP + j];
                bacc += s;
            }
            if (l > 0) {
                tr_backward_layer(prm + net.oW[l], d[l], d[l + 1], dz, dh, wave, lane);
                __syncthreads();
                // through the PReLU of layer l's input: dz = z > 0 ? dh : a dh; d slope = sum over z <= 0 of z dh (torch's prelu backward)
                for (int e = t; e < d[l] * kTrTS; e += kTrThreads) {
                    const int k = e / kTrTS, s = e % kTrTS;
                    const float z = zin[k * kTrSP + s], g = dh[k * kTrSP + s];
                    const bool pos = z > 0.0f;
                    dh[k * kTrSP + s] = pos ? g : slope_in * g;
                    sacc[l - 1] += pos ? 0.0f : z * g;
                }
            }
            __syncthreads();
        }
    }
    // the workgroup's partial, torch layout + the loss sum at [P]
    float *out = partial + (size_t)blockIdx.x * net.Pp;
#pragma unroll
    for (int l = 0; l < 5; l++) {
        const int KT = (d[l] + 31) / 32, dn = d[l + 1], dk = d[l];
#pragma unroll
        for (int m = 0; m < kTrMaxTiles; m++) {
            const int g = m * kTrWaves + wave;
            if (g >= tbase[l] && g < tbase[l + 1]) {
                const int n0 = ((g - tbase[l]) / KT) * 32, k = ((g - tbase[l]) % KT) * 32 + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = n0 + tr_row(r, lane);
                    if (n < dn && k < dk) out[net.oW[l] + n * dk + k] = acc[m][r];
                }
            }
        }
        if (t >= bbase[l] && t < bbase[l + 1]) out[net.oB[l] + t - bbase[l]] = bacc;
    }
    // slopes and loss: fixed-shape tree sums over the workgroup
    float *red = lds;
    __syncthreads();
    for (int q = 0; q < 5; q++) {
        tr_block_sum(q < 4 ? sacc[q] : lacc, red, t);
        if (t == 0) out[q < 4 ? net.oA[q] : net.P] = red[0];
        __syncthreads();
    }
}
template <class ROW>
__global__ __launch_bounds__(kTrThreads) void k_train_grad(TrainRing ring, TrainNet net, const float *__restrict__ prm, const float *__restrict__ tgt,
                                                           const int32_t *__restrict__ lists, const int32_t *__restrict__ counts, int64_t N, int agent,
                                                           int team, float gamma, float *__restrict__ partial, float *step) {
    extern __shared__ float lds[];
    tr_grad<ROW>(ring, net, prm, tgt, lists, counts, N, agent, team, gamma, partial, step, lds);
}
template <class ROW>
__global__ __launch_bounds__(kTrThreads) void k_train_sweep_grad(TrainTable tab, TrainNet net, int64_t N, int agent, int team) {
    extern __shared__ float lds[];
    const TrainLearner &a = tab.l[blockIdx.y];
    tr_grad<ROW>(a.ring, net, a.prm, a.tgt, a.lists, a.counts, N, agent, team, a.gamma, a.partial, a.step, lds);
}


// ---- k_train_adam: thread per parameter (tr_adam); the single-learner form serves the dense learner's stacks too ----
__global__ __launch_bounds__(256) void k_train_adam(int P, int Pp, const int32_t *__restrict__ counts, int agent, int team, const float *__restrict__ partial,
                                                    int G, float *__restrict__ gacc, float *__restrict__ prm, float *__restrict__ m1, float *__restrict__ m2,
                                                    const float *__restrict__ step, double lr, double beta1, double beta2, double eps, float *losses) {
    tr_adam(P, Pp, counts, agent, team, partial, G, gacc, prm, m1, m2, step, lr, beta1, beta2, eps, losses);
}
__global__ __launch_bounds__(256) void k_train_sweep_adam(TrainTable tab, TrainNet net, int agent, int team, int G) {
    const TrainLearner &a = tab.l[blockIdx.y];
    tr_adam(net.P, net.Pp, a.counts, agent, team, a.partial, G, a.gacc, a.prm, a.m1, a.m2, a.step, a.lr, a.beta1, a.beta2, a.eps, a.losses);
}

// ---- k_train_pack: the team's packed image from torch-layout parameters (susnet_capi_nets.hip qnet_pack, element for element) ----
template <class ROW>
__device__ __forceinline__ void tr_pack(const TrainNet &net, const float *__restrict__ prm, float *__restrict__ out) {
    using Q = QNet<ROW>;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q::kPacked) return;
    const int *d = net.d;
    const float *W1 = prm + net.oW[0], *B1 = prm + net.oB[0];
    float v = 0.0f;
    if (i < Q::oB2) {
        const int row = i / Q::kRowStride, n = i % Q::kRowStride;
        if (row < Q::kRows && n < d[1]) {
            if (row < Q::kOneHot) {
                if constexpr (ROW::kDeadZero) v = W1[(size_t)n * Q::F + row];
                else v = (float)(row % ROW::N) * W1[(size_t)n * Q::F + row / ROW::N];
            } else if (row >= Q::kTail) {
                const int bits = row - Q::kTail;
                float a = B1[n];
                for (int bit = 0; bit < Q::kTailBits; bit++)
                    if ((bits >> bit) & 1) a += W1[(size_t)n * Q::F + (Q::F - Q::kTailBits) + bit];
                v = a;
            }
        }
    } else if (i < Q::oW2) {
        const int ob[5] = {Q::oB2, Q::oB3, Q::oB4, Q::oB5, Q::oW2};
        for (int l = 1; l < 5; l++)
            if (i >= ob[l - 1] && i < ob[l]) {
                const int n = i - ob[l - 1];
                v = n < d[l + 1] ? prm[net.oB[l] + n] : 0.0f;
            }
    } else if (i < Q::oSlope) {
        const int ow[5] = {Q::oW2, Q::oW3, Q::oW4, Q::oW5, Q::oSlope};
        const int pad[6] = {Q::F, Q::H1, Q::H2, Q::H3, Q::H4, Q::NO};
        for (int l = 1; l < 5; l++)
            if (i >= ow[l - 1] && i < ow[l]) { // qnet_pack_dense's index, inverted
                const int u = i - ow[l - 1], NB = pad[l + 1] / 32;
                const int r = u & 3, ln = (u >> 2) & 63, q = (u >> 8) & 3, blk = u >> 10;
                const int kb = blk / NB, nb = blk % NB;
                const int n = 32 * nb + (ln & 31), k = 32 * kb + 8 * q + 4 * (ln >> 5) + r;
                v = (n < d[l + 1] && k < d[l]) ? prm[net.oW[l] + (size_t)n * d[l] + k] : 0.0f;
            }
    } else {
        v = prm[net.oA[i - Q::oSlope]];
    }
    out[i] = v;
}
template <class ROW>
__global__ __launch_bounds__(256) void k_train_pack(TrainNet net, const float *__restrict__ prm, float *__restrict__ out) {
    tr_pack<ROW>(net, prm, out);
}
template <class ROW>
__global__ __launch_bounds__(256) void k_train_sweep_pack(TrainTable tab, TrainNet net) { // (a learner without a packed image: nothing to write)
    const TrainLearner &a = tab.l[blockIdx.y];
    if (a.packed) tr_pack<ROW>(net, a.prm, a.packed);
}

} // namespace susnet
