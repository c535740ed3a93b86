// susnet_dropout.h -- the dropout mask between the layers of nn.RNN (training mode, dropout = p, num_layers > 1), as the dropout form of
// the SpatialDQN train step applies it (susnet_spatial_train_step_dropout) and susnet_rnn_dropout_mask writes it out.  ONE device
// function, sp_drop4 below: the multiplier of (net, agent, row, t, layer, unit) is a pure function of those six, the seed and the offset
// -- include/susnet.h states the counter and key layout -- so it does not depend on the grid, the tile, the wave or the order of a list.
// The train step generates a tile's multipliers once, at the tanh write, and keeps them in its workspace for the next layer's operands,
// the backward pass and the weight gradient; susnet_rnn_dropout_mask's kernel generates the same values.  The acting forward under
// dropout (k_spatial_rnn_dropout, susnet_spatial.h) evaluates the same function at its own coordinates (sp_drop4_at, SpActDrop below:
// nets 2 / 3), also at the tanh write, and keeps the PRODUCT m h in LDS for the next layer; susnet_spatial_act_dropout_mask writes those multipliers out.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/susnet.h"

namespace susnet {

struct SpDrop { // by value: part of a dropout kernel's arguments
    uint32_t k0, k1;         // the key: seed lo, hi
    uint32_t off_lo, off_hi; // offset (off_hi < 2^24)
    uint32_t thr[2];         // per net (0 online, 1 target): floor(p 2^32); an element is kept iff its word >= thr.  0: no mask
    float scale[2];          // per net: 1.0f / (1.0f - p)
    int64_t row_base;
    int32_t agent;
};

#ifdef __HIPCC__
// Philox4x32-10 on one counter block (the rounds of PhiloxRng::gen, susnet_device.h)
__device__ __forceinline__ void sp_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// the multipliers of units 4 q .. 4 q + 3 (one Philox block; word j belongs to unit 4 q + j) of `row` (row_base not yet added) at step t
// behind layer `layer`: 0 or scale[net].  thr[net] == 0 (floor(p 2^32) == 0): 1.0f, no block generated
__device__ __forceinline__ void sp_drop4(const SpDrop &d, int net, int64_t row, int t, int layer, int q, float (&m)[4]) {
    const uint32_t thr = d.thr[net];
    if (thr == 0u) {
        m[0] = m[1] = m[2] = m[3] = 1.0f;
        return;
    }
    const uint64_t g = (uint64_t)(d.row_base + row);
    uint32_t w[4];
    sp_philox(d.k0, d.k1, (uint32_t)q | (uint32_t)layer << 8 | (uint32_t)t << 12 | (uint32_t)net << 16 | (uint32_t)d.agent << 20, (uint32_t)g,
              ((uint32_t)(g >> 32) & 0xFFu) | d.off_hi << 8, d.off_lo, w);
    const float s = d.scale[net];
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = w[j] >= thr ? s : 0.0f;
}

// the same function of (net, agent, row G) given one by one, for the acting forward, whose agent and row differ from lane to lane (SpActDrop
// below): the counter and the keep rule are sp_drop4's, word for word.  (sp_drop4 is not written as a call of this one: passed thr[net] and
// scale[net] as values, the train step's kernels index the by-value struct through scratch memory, which the build refuses.)
__device__ __forceinline__ void sp_drop4_at(uint32_t k0, uint32_t k1, uint32_t off_lo, uint32_t off_hi, uint32_t thr, float scale, int net, int agent,
                                            uint64_t g, int t, int layer, int q, float (&m)[4]) {
    if (thr == 0u) {
        m[0] = m[1] = m[2] = m[3] = 1.0f;
        return;
    }
    uint32_t w[4];
    sp_philox(k0, k1, (uint32_t)q | (uint32_t)layer << 8 | (uint32_t)t << 12 | (uint32_t)net << 16 | (uint32_t)agent << 20, (uint32_t)g,
              ((uint32_t)(g >> 32) & 0xFFu) | off_hi << 8, off_lo, w);
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = w[j] >= thr ? scale : 0.0f;
}
#endif

// the acting forward's coordinates (susnet_spatial_forward_dropout, susnet_spatial_act_dropout_mask): row r of the call is
// (agent r % agents, row G = row_base + r / agents: the env), net 2 the imposters' acting network, 3 the crew's
struct SpActDrop { // by value: part of the kernels' arguments
    uint32_t k0, k1, off_lo, off_hi;
    uint32_t thr; // floor(p 2^32), not 0: the p == 0 forms launch the plain kernels
    float scale;  // 1.0f / (1.0f - p)
    int64_t row_base;
    int32_t agents, net;
};

// host: one susnet_rnn_dropout (`who` names it: "drop->", "drop[1].") checked for a call that masks `rows` rows, and turned into kernel
// arguments.  BAD: susnet_host.h's Refuse
template <class BAD>
inline int drop_check(const BAD &bad, const std::string &who, const susnet_rnn_dropout &d, int64_t rows, SpDrop &out) {
    out = SpDrop{};
    for (int net = 0; net < 2; net++) {
        const float p = d.p[net];
        if (!(p >= 0.0f && p < 1.0f)) return bad(who + "p[" + std::to_string(net) + "] = " + std::to_string(p) + " (served: 0 <= p < 1)");
        out.thr[net] = (uint32_t)((double)p * 4294967296.0); // floor: p < 1 in float32 is at most 1 - 2^-24
        out.scale[net] = 1.0f / (1.0f - p);
    }
    if (d.offset >> 56) return bad(who + "offset = " + std::to_string((unsigned long long)d.offset) + " (served: below 2^56)");
    if (d.row_base < 0 || d.row_base > (1ll << 40) - rows)
        return bad(who + "row_base = " + std::to_string((long long)d.row_base) + " (served: row_base >= 0, row_base + rows <= 2^40)");
    out.k0 = (uint32_t)d.seed, out.k1 = (uint32_t)(d.seed >> 32);
    out.off_lo = (uint32_t)d.offset, out.off_hi = (uint32_t)(d.offset >> 32);
    out.row_base = d.row_base;
    return 0;
}

// susnet_rnn_dropout_mask's kernel (inst_qnet_spatial.hip): out [layers - 1][n][T][H]
hipError_t rnn_dropout_mask_launch(const SpDrop &d, int net, int layers, int64_t n, int T, int H, float *out, hipStream_t st);
// susnet_spatial_act_dropout_mask's kernel (inst_qnet_spatial.hip): out [layers - 1][n][T][H] of the acting rows 0 .. n - 1
hipError_t act_dropout_mask_launch(const SpActDrop &d, int layers, int64_t n, int T, int H, float *out, hipStream_t st);

} // namespace susnet
