// susnet_capi_nets.hip -- the network entry points of the C ABI, none of which touches a stepping kernel: the compiled-in Q-network's checks,
// pack and forward (qnet_feat and qnet_dims_ok serve the one-kernel tick of susnet_capi.hip and the fused learner of susnet_capi_train.hip
// too), susnet_mlp_forward, susnet_spatial_forward and susnet_window_push.  Their kernels: inst_qnet_*.hip and inst_window.hip.  What a
// Linear / PReLU stack and a SpatialDQN are checked for, and how a stack becomes kernel arguments, is stated once, in susnet_host.h.
#include <algorithm>

#include "susnet_qnet.h"
#include "susnet_dense.h"
#include "susnet_spatial.h"
#include "susnet_dropout.h"
#include "susnet_window.h"
#include "susnet_host.h"

using namespace susnet;

// ---- the policy loop's Q-network (susnet_qnet.h) ----
// which compiled-in feature layout (susnet_flat.h) a component list on this handle is: 0 = none (susnet_capi.hip and susnet_capi_train.hip ask too)
int qnet_feat(const susnet_env *env, const int32_t *comp, int32_t ncomp) {
    if (!env || !comp) return 0;
    const Consts &c = env->c;
    if (c.A == 2 && c.N == 9 && ncomp == 1 && comp[0] == SUSNET_F_ONEHOT_POS) return FEAT_ONEHOT;
    if (c.A == 2 && c.N == 9 && ncomp == 1 && comp[0] == SUSNET_F_COORD_POS) return FEAT_COORD;
    if (c.A == 3 && c.N == 14 && c.n_imp == 1 && ncomp == 3 && comp[0] == SUSNET_F_ONEHOT_POS && comp[1] == SUSNET_F_ALIVE_CREW &&
        comp[2] == SUSNET_F_CLOSEST_CREW)
        return FEAT_ONEHOT_ALIVE_CLOSEST;
    return 0;
}
template <class ROW>
bool qnet_dims_ok(const int32_t *dims, int32_t n_dims) {
    using Q = QNet<ROW>;
    const int cap[6] = {Q::F, Q::H1, Q::H2, Q::H3, Q::H4, Q::NO};
    if (!dims || n_dims != 6 || dims[0] != Q::F) return false;
    for (int l = 1; l < 6; l++)
        if (dims[l] < 1 || dims[l] > cap[l]) return false;
    return true;
}
template bool qnet_dims_ok<QRow1>(const int32_t *, int32_t);
template bool qnet_dims_ok<QRow3>(const int32_t *, int32_t);
template bool qnet_dims_ok<QRowC>(const int32_t *, int32_t);
// torch Linear weight [dn][dk] -> 32 x 32 blocks in [kb][nb] order; inside a block lane l holds, as four float4, the 16 k values of row
// n = 32 nb + l % 32 in MFMA-step order: float4 q = columns 32 kb + 8 q + 4 (l / 32) + {0, 1, 2, 3}
static void qnet_pack_dense(const float *W, int dk, int dn, int KP, int NP, float *dst) {
    const int KB = KP / 32, NB = NP / 32;
    for (int kb = 0; kb < KB; kb++)
        for (int nb = 0; nb < NB; nb++)
            for (int q = 0; q < 4; q++)
                for (int l = 0; l < 64; l++)
                    for (int r = 0; r < 4; r++) {
                        const int n = 32 * nb + (l & 31), k = 32 * kb + 8 * q + 4 * (l >> 5) + r;
                        dst[((((size_t)kb * NB + nb) * 4 + q) * 64 + l) * 4 + r] = (n < dn && k < dk) ? W[(size_t)n * dk + k] : 0.0f;
                    }
}
template <class ROW>
static void qnet_pack(const int32_t *d, const float *const *W, const float *const *Bv, const float *slopes, float *out) {
    using Q = QNet<ROW>;
    std::fill(out, out + Q::kPacked, 0.0f);
    // layer 1, transposed: one row per position bit (row kZero stays zero) ...
    if constexpr (ROW::kDeadZero) {
        for (int f = 0; f < Q::kOneHot; f++)
            for (int n = 0; n < d[1]; n++) out[Q::oW1 + f * Q::kRowStride + n] = W[0][(size_t)n * Q::F + f];
    } else { // ... the coordinate layout: row (coordinate c, value k) = k x column c of W1 (one float32 rounding, as torch's product has)
        for (int cc = 0; cc < Q::F; cc++)
            for (int k = 0; k < ROW::N; k++)
                for (int n = 0; n < d[1]; n++) out[Q::oW1 + (cc * ROW::N + k) * Q::kRowStride + n] = (float)k * W[0][(size_t)n * Q::F + cc];
    }
    // ... and one per combination v of the bits behind the one-hots: b1 + the columns of v's set bits, lowest first (float32 sums)
    for (int v = 0; v < (1 << Q::kTailBits); v++)
        for (int n = 0; n < d[1]; n++) {
            float acc = Bv[0][n];
            for (int bit = 0; bit < Q::kTailBits; bit++)
                if ((v >> bit) & 1) acc += W[0][(size_t)n * Q::F + (Q::F - Q::kTailBits) + bit];
            out[Q::oW1 + (Q::kTail + v) * Q::kRowStride + n] = acc;
        }
    const int off_w[4] = {Q::oW2, Q::oW3, Q::oW4, Q::oW5}, off_b[4] = {Q::oB2, Q::oB3, Q::oB4, Q::oB5};
    const int pad[6] = {Q::F, Q::H1, Q::H2, Q::H3, Q::H4, Q::NO};
    for (int l = 1; l < 5; l++) {
        qnet_pack_dense(W[l], d[l], d[l + 1], pad[l], pad[l + 1], out + off_w[l - 1]);
        for (int n = 0; n < d[l + 1]; n++) out[off_b[l - 1] + n] = Bv[l][n];
    }
    for (int l = 0; l < 4; l++) out[Q::oSlope + l] = slopes[l];
}
// (the kernels live in translation units of their own: inst_qnet_*.hip)
namespace susnet {
SUSNET_QNET_FOR(extern, QRow1, QSpec2)
SUSNET_QNET_FOR(extern, QRow3, QSpec3)
SUSNET_QNET_FOR(extern, QRowC, QSpec2)
}

extern "C" int64_t susnet_qnet_packed_floats(const susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims,
                                             int32_t n_dims) {
    switch (qnet_feat(env, components, n_components)) {
    case FEAT_ONEHOT: if (qnet_dims_ok<QRow1>(dims, n_dims)) return QNet<QRow1>::kPacked; break;
    case FEAT_ONEHOT_ALIVE_CLOSEST: if (qnet_dims_ok<QRow3>(dims, n_dims)) return QNet<QRow3>::kPacked; break;
    case FEAT_COORD: if (qnet_dims_ok<QRowC>(dims, n_dims)) return QNet<QRowC>::kPacked; break;
    }
    return fail(SUSNET_E_INVALID, "susnet_qnet: served are five Linear layers [F, <=256, <=128, <=64, <=32, <=32] on the compiled-in feature "
                                  "layouts (onehot_pos or coord_pos on the 2-agent 9x9 game; onehot_pos + alive_crew + closest_crew on the 3-agent 14x14 game)");
}

extern "C" int susnet_qnet_pack(const susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims, int32_t n_dims,
                                const float *const *weights, const float *const *biases, const float *slopes, float *packed) {
    const int64_t n = susnet_qnet_packed_floats(env, components, n_components, dims, n_dims);
    if (n < 0) return (int)n;
    if (!weights || !biases || !slopes || !packed) return fail(SUSNET_E_INVALID, "susnet_qnet_pack: null weights / biases / slopes / packed");
    for (int l = 0; l < 5; l++)
        if (!weights[l] || !biases[l]) return fail(SUSNET_E_INVALID, "susnet_qnet_pack: null layer");
    switch (qnet_feat(env, components, n_components)) {
    case FEAT_ONEHOT: qnet_pack<QRow1>(dims, weights, biases, slopes, packed); break;
    case FEAT_COORD: qnet_pack<QRowC>(dims, weights, biases, slopes, packed); break;
    default: qnet_pack<QRow3>(dims, weights, biases, slopes, packed); break;
    }
    return SUSNET_OK;
}

template <class ROW>
static int qnet_launch(susnet_env *env, const float *packed, float *q_out, int n_out, hipStream_t st) {
    HIP_TRY((qnet_launch_k<ROW>(env->c, env->s, packed, q_out, n_out, st)));
    return SUSNET_OK;
}
extern "C" int susnet_qnet_forward(susnet_env *env, const int32_t *components, int32_t n_components, const int32_t *dims, int32_t n_dims,
                                   const float *packed, float *q_out, void *stream) {
    if (int rc = check_bound(env)) return rc;
    const int64_t n = susnet_qnet_packed_floats(env, components, n_components, dims, n_dims);
    if (n < 0) return (int)n;
    if (!packed || !q_out || (reinterpret_cast<uintptr_t>(packed) & 15u)) return fail(SUSNET_E_INVALID, "susnet_qnet_forward: packed (16-byte aligned) / q_out");
    switch (qnet_feat(env, components, n_components)) {
    case FEAT_ONEHOT: return qnet_launch<QRow1>(env, packed, q_out, dims[5], static_cast<hipStream_t>(stream));
    case FEAT_COORD: return qnet_launch<QRowC>(env, packed, q_out, dims[5], static_cast<hipStream_t>(stream));
    default: return qnet_launch<QRow3>(env, packed, q_out, dims[5], static_cast<hipStream_t>(stream));
    }
}

// susnet_mlp_forward: any served layer stack on caller-supplied rows (the kernel: inst_qnet_dense.hip).  Everything is checked here, before
// the launch; the handle gives the error conventions only (no state is read: it need not be bound).
extern "C" int susnet_mlp_forward(susnet_env *env, const susnet_mlp_io *io, void *stream) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_mlp_forward: null env / io");
    const Refuse bad{env, "susnet_mlp_forward"};
    if (int rc = check_stack_n_dims(bad, "", io->n_dims)) return rc;
    if (int rc = check_feature_width(bad, "", io->dims[0])) return rc;
    if (int rc = check_stack_dims(bad, "", io->n_dims, io->dims, kDnMaxHidden, kDnMaxOut)) return rc;
    if (io->n < 1) return bad("n = " + std::to_string((long long)io->n) + " (at least one row)");
    if (int rc = check_stack_ptrs(bad, "", io->n_dims - 1, io->weight, io->bias, io->slope)) return rc;
    if (!io->rows || misaligned(io->rows)) return bad("rows is NULL or not 4-byte aligned");
    if (!io->q_out || misaligned(io->q_out)) return bad("q_out is NULL or not 4-byte aligned");
    DenseArgs a{};
    fill_stack(a, *io);
    a.rows = io->rows;
    a.n = io->n;
    a.q = io->q_out;
    HIP_TRY(qnet_dense_launch(a, static_cast<hipStream_t>(stream)));
    return SUSNET_OK;
}

// susnet_spatial_forward: SpatialDQN.forward in eval mode (the kernels: inst_qnet_spatial.hip).  Everything is checked here, before the first
// launch; the handle gives the error conventions only.
// susnet_spatial_forward_dropout (act != nullptr) is the same call with nn.RNN's training-mode dropout between the layers: the same checks
// with the same messages behind its own name, then the mask's (drop->p[net - 2], offset, row_base over the call's envs, agents) and the
// LDS rule of the form that is launched -- the plain kernels' where floor(p 2^32) == 0 or there is one layer.
struct SpatialAct {
    const susnet_rnn_dropout *drop;
    int32_t net; // 2 the imposters' acting network, 3 the crew's
};
static int spatial_forward(susnet_env *env, const susnet_spatial_io *io, const char *entry, const SpatialAct *act, void *stream) {
    const Refuse bad{env, entry};
    const auto S = [](long long v) { return std::to_string(v); };
    if (act) {
        if (!act->drop) return bad("drop is NULL");
        if (act->net < 2 || act->net > 3) return bad("net = " + S(act->net) + " (served: 2 .. 3, the imposters' and the crew's acting network)");
    }
    SpatialGeom g;
    if (int rc = check_spatial_net(bad, "", "", *io, io->n_dims, io->dims, kDnMaxHidden, kDnMaxOut, g)) return rc;
    if (io->n < 1) return bad("n = " + S(io->n) + " (at least one row)");
    if (io->n > (INT64_MAX >> 20)) return bad("n = " + S(io->n) + " (the workspace's byte count overflows)");
    if (io->agents < 1) return bad("agents = " + S(io->agents) + " (at least one agent per env)");
    for (int d = 0; d < 3; d++) {
        if (io->spatial_stride[d] < 0) return bad("spatial_stride[" + S(d) + "] = " + S(io->spatial_stride[d]) + " (at least 0)");
        if (io->Fn > 0 && io->non_spatial_stride[d] < 0) return bad("non_spatial_stride[" + S(d) + "] = " + S(io->non_spatial_stride[d]) + " (at least 0)");
    }
    for (int l = 0; l < io->n_conv; l++) {
        const std::string at = "[" + S(l) + "]";
        if (!io->conv_weight[l] || misaligned(io->conv_weight[l])) return bad("conv_weight" + at + " is NULL or not 4-byte aligned");
        if (!io->conv_bias[l] || misaligned(io->conv_bias[l])) return bad("conv_bias" + at + " is NULL or not 4-byte aligned");
    }
    for (int l = 0; l < io->rnn_layers; l++) {
        const std::string at = "[" + S(l) + "]";
        if (!io->w_ih[l] || misaligned(io->w_ih[l])) return bad("w_ih" + at + " is NULL or not 4-byte aligned");
        if (!io->w_hh[l] || misaligned(io->w_hh[l])) return bad("w_hh" + at + " is NULL or not 4-byte aligned");
        if (!io->b_ih[l] || misaligned(io->b_ih[l])) return bad("b_ih" + at + " is NULL or not 4-byte aligned");
        if (!io->b_hh[l] || misaligned(io->b_hh[l])) return bad("b_hh" + at + " is NULL or not 4-byte aligned");
    }
    if (int rc = check_stack_ptrs(bad, "", io->n_dims - 1, io->weight, io->bias, io->slope)) return rc;
    if (!io->spatial || misaligned(io->spatial)) return bad("spatial is NULL or not 4-byte aligned");
    // (Fn = 0: nothing is read through non_spatial, so NULL is accepted -- a [B][T][0] tensor has no storage; a pointer that is given is still checked)
    if ((!io->non_spatial && io->Fn > 0) || misaligned(io->non_spatial)) return bad("non_spatial is NULL or not 4-byte aligned");
    if (!io->rnn_in || misaligned(io->rnn_in)) return bad("rnn_in is NULL or not 4-byte aligned");
    if (!io->q_out || misaligned(io->q_out)) return bad("q_out is NULL or not 4-byte aligned");
    SpatialConvArgs ca{};
    ca.T = io->T;
    ca.C = io->C;
    ca.n_conv = io->n_conv;
    ca.k = io->k;
    ca.Fn = io->Fn;
    ca.agents = io->agents;
    ca.R = g.R;
    for (int l = 0; l <= io->n_conv; l++) ca.size[l] = g.size[l];
    for (int l = 0; l < io->n_conv; l++) {
        ca.co[l] = io->conv_out[l];
        ca.stride[l] = io->conv_stride[l];
        ca.pad[l] = io->conv_padding[l];
        ca.dil[l] = io->conv_dilation[l];
        ca.W[l] = io->conv_weight[l];
        ca.B[l] = io->conv_bias[l];
    }
    ca.spatial = io->spatial;
    ca.non_spatial = io->non_spatial;
    for (int d = 0; d < 3; d++) {
        ca.sp_stride[d] = io->spatial_stride[d];
        ca.ns_stride[d] = io->Fn > 0 ? io->non_spatial_stride[d] : 0; // (Fn = 0: the strides are not looked at)
    }
    ca.n = io->n;
    ca.rnn_in = io->rnn_in;
    SpatialRnnArgs ra{};
    ra.T = io->T;
    ra.R = g.R;
    ra.L = io->rnn_layers;
    ra.H = io->rnn_hidden;
    for (int l = 0; l < io->rnn_layers; l++) {
        ra.w_ih[l] = io->w_ih[l];
        ra.w_hh[l] = io->w_hh[l];
        ra.b_ih[l] = io->b_ih[l];
        ra.b_hh[l] = io->b_hh[l];
    }
    fill_stack(ra, *io);
    ra.rnn_in = io->rnn_in;
    ra.n = io->n;
    ra.q = io->q_out;
    SpActDrop dr{};
    if (act) {
        const susnet_rnn_dropout &d = *act->drop;
        const int team = act->net - 2;
        const float p = d.p[team];
        if (!(p >= 0.0f && p < 1.0f)) return bad("drop->p[" + S(team) + "] = " + std::to_string(p) + " (served: 0 <= p < 1)");
        if (d.offset >> 56) return bad("drop->offset = " + std::to_string((unsigned long long)d.offset) + " (served: below 2^56)");
        const int64_t envs = (io->n + io->agents - 1) / io->agents;
        if (d.row_base < 0 || d.row_base > (1ll << 40) - envs)
            return bad("drop->row_base = " + S(d.row_base) + " (served: row_base >= 0, row_base + n / agents <= 2^40)");
        if (io->agents > 4096) return bad("agents = " + S(io->agents) + " (served under dropout: at most 4096, the mask's agent coordinate)");
        dr.thr = (uint32_t)((double)p * 4294967296.0); // floor, as drop_check (susnet_dropout.h)
        dr.scale = 1.0f / (1.0f - p);
        dr.k0 = (uint32_t)d.seed, dr.k1 = (uint32_t)(d.seed >> 32);
        dr.off_lo = (uint32_t)d.offset, dr.off_hi = (uint32_t)(d.offset >> 32);
        dr.row_base = d.row_base;
        dr.agents = io->agents;
        dr.net = act->net;
    }
    const bool dropout = act && dr.thr != 0u && io->rnn_layers > 1; // else: susnet_spatial_forward's kernels, bit for bit
    const size_t conv_lds = spatial_conv_lds(ca), rnn_lds = dropout ? spatial_rnn_dropout_lds(ra) : spatial_rnn_lds(ra);
    if (conv_lds > kSpLdsBudget)
        return bad("LDS: one image's activation buffers take " + S((long long)conv_lds) + " bytes of a workgroup's " + S((long long)kSpLdsBudget) +
                   " (C, N, conv_out, conv_padding)");
    if (rnn_lds > kSpLdsBudget)
        return bad(std::string(dropout ? (io->rnn_layers > 2 ? "LDS under dropout: (rnn_layers + 3)" : "LDS under dropout: (rnn_layers + 2)") : "LDS: (rnn_layers + 1)") +
                   " x 64 rows x max(rnn_hidden, head widths) floats = " + S((long long)rnn_lds) + " bytes of a workgroup's " + S((long long)kSpLdsBudget));
    HIP_TRY(spatial_conv_launch(ca, static_cast<hipStream_t>(stream)));
    if (dropout)
        HIP_TRY(spatial_rnn_dropout_launch(ra, dr, static_cast<hipStream_t>(stream)));
    else
        HIP_TRY(spatial_rnn_launch(ra, static_cast<hipStream_t>(stream)));
    return SUSNET_OK;
}

extern "C" int susnet_spatial_forward(susnet_env *env, const susnet_spatial_io *io, void *stream) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_spatial_forward: null env / io");
    return spatial_forward(env, io, "susnet_spatial_forward", nullptr, stream);
}

extern "C" int susnet_spatial_forward_dropout(susnet_env *env, const susnet_spatial_io *io, const susnet_rnn_dropout *drop, int32_t net, void *stream) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_spatial_forward_dropout: null env / io");
    const SpatialAct act{drop, net};
    return spatial_forward(env, io, "susnet_spatial_forward_dropout", &act, stream);
}

// susnet_rnn_dropout_mask: the multipliers susnet_spatial_train_step_dropout applies, written out (the kernel: inst_qnet_spatial.hip)
extern "C" int susnet_rnn_dropout_mask(susnet_env *env, const susnet_rnn_dropout *drop, int32_t net, int32_t agent, int32_t layers, int64_t n,
                                       int32_t T, int32_t H, float *out, void *stream) {
    if (!env) return fail(SUSNET_E_INVALID, "susnet_rnn_dropout_mask: null env");
    const Refuse bad{env, "susnet_rnn_dropout_mask"};
    const auto range = [&](const char *field, long long v, long long lo, long long hi) {
        return std::string(field) + " = " + std::to_string(v) + " (served: " + std::to_string(lo) + " .. " + std::to_string(hi) + ")";
    };
    if (!drop) return bad("drop is NULL");
    if (net < 0 || net > 1) return bad(range("net", net, 0, 1));
    if (agent < 0 || agent > 4095) return bad(range("agent", agent, 0, 4095));
    if (layers < 2 || layers > kSpMaxRnn) return bad(range("layers", layers, 2, kSpMaxRnn));
    if (n < 1 || n > (1ll << 40)) return bad(range("n", n, 1, 1ll << 40));
    if (T < 1 || T > SUSNET_SPATIAL_MAX_T) return bad(range("T", T, 1, SUSNET_SPATIAL_MAX_T));
    if (H < 1 || H > kDnMaxHidden) return bad(range("H", H, 1, kDnMaxHidden));
    SpDrop dr{};
    if (int rc = drop_check(bad, "drop->", *drop, n, dr)) return rc;
    if (!out || misaligned(out)) return bad("out is NULL or not 4-byte aligned");
    dr.agent = agent;
    HIP_TRY(rnn_dropout_mask_launch(dr, net, layers, n, T, H, out, static_cast<hipStream_t>(stream)));
    return SUSNET_OK;
}

// susnet_spatial_act_dropout_mask: the multipliers susnet_spatial_forward_dropout applies to rows 0 .. n - 1 of a call with `agents`
extern "C" int susnet_spatial_act_dropout_mask(susnet_env *env, const susnet_rnn_dropout *drop, int32_t net, int32_t agents, int32_t layers, int64_t n,
                                               int32_t T, int32_t H, float *out, void *stream) {
    if (!env) return fail(SUSNET_E_INVALID, "susnet_spatial_act_dropout_mask: null env");
    const Refuse bad{env, "susnet_spatial_act_dropout_mask"};
    const auto range = [&](const char *field, long long v, long long lo, long long hi) {
        return std::string(field) + " = " + std::to_string(v) + " (served: " + std::to_string(lo) + " .. " + std::to_string(hi) + ")";
    };
    if (!drop) return bad("drop is NULL");
    if (net < 2 || net > 3) return bad(range("net", net, 2, 3));
    if (agents < 1 || agents > 4096) return bad(range("agents", agents, 1, 4096));
    if (layers < 2 || layers > kSpMaxRnn) return bad(range("layers", layers, 2, kSpMaxRnn));
    if (n < 1 || n > (1ll << 40)) return bad(range("n", n, 1, 1ll << 40));
    if (T < 1 || T > SUSNET_SPATIAL_MAX_T) return bad(range("T", T, 1, SUSNET_SPATIAL_MAX_T));
    if (H < 1 || H > kDnMaxHidden) return bad(range("H", H, 1, kDnMaxHidden));
    const float p = drop->p[net - 2];
    if (!(p >= 0.0f && p < 1.0f)) return bad("drop->p[" + std::to_string(net - 2) + "] = " + std::to_string(p) + " (served: 0 <= p < 1)");
    if (drop->offset >> 56) return bad("drop->offset = " + std::to_string((unsigned long long)drop->offset) + " (served: below 2^56)");
    const int64_t envs = (n + agents - 1) / agents;
    if (drop->row_base < 0 || drop->row_base > (1ll << 40) - envs)
        return bad("drop->row_base = " + std::to_string((long long)drop->row_base) + " (served: row_base >= 0, row_base + n / agents <= 2^40)");
    if (!out || misaligned(out)) return bad("out is NULL or not 4-byte aligned");
    SpActDrop dr{};
    dr.thr = (uint32_t)((double)p * 4294967296.0);
    dr.scale = 1.0f / (1.0f - p);
    dr.k0 = (uint32_t)drop->seed, dr.k1 = (uint32_t)(drop->seed >> 32);
    dr.off_lo = (uint32_t)drop->offset, dr.off_hi = (uint32_t)(drop->offset >> 32);
    dr.row_base = drop->row_base;
    dr.agents = agents;
    dr.net = net;
    HIP_TRY(act_dropout_mask_launch(dr, layers, n, T, H, out, static_cast<hipStream_t>(stream)));
    return SUSNET_OK;
}

// susnet_window_push: the feature window of the acting loop, one tick on (the kernel: inst_window.hip).  Everything is checked here, before
// the launch; as for susnet_mlp_forward the handle gives the error conventions only (no state is read: it need not be bound).
extern "C" int susnet_window_push(susnet_env *env, const susnet_window_io *io, void *stream) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_window_push: null env / io");
    const Refuse bad{env, "susnet_window_push"};
    if (io->T < 1 || io->T > kWinMaxT) return bad("T = " + std::to_string(io->T) + " (served: 1 .. " + std::to_string(kWinMaxT) + " states per window)");
    if (io->F < 1) return bad("F = " + std::to_string(io->F) + " (at least one feature per state)");
    if ((int64_t)io->T * io->F > SUSNET_MLP_MAX_F)
        return bad("T * F = " + std::to_string((long long)io->T * io->F) + " (a window is one input row of susnet_mlp_forward: at most SUSNET_MLP_MAX_F = " +
                   std::to_string(SUSNET_MLP_MAX_F) + ")");
    if (io->n < 1) return bad("n = " + std::to_string((long long)io->n) + " (at least one row)");
    if (io->n > (INT64_MAX >> 13)) return bad("n = " + std::to_string((long long)io->n) + " (the window's byte count overflows)");
    if (!io->fresh || misaligned(io->fresh)) return bad("fresh is NULL or not 4-byte aligned");
    if (!io->src || misaligned(io->src)) return bad("src is NULL or not 4-byte aligned");
    if (!io->dst || misaligned(io->dst)) return bad("dst is NULL or not 4-byte aligned");
    const uintptr_t wbytes = (uintptr_t)io->n * (uintptr_t)io->T * (uintptr_t)io->F * 4u, fbytes = (uintptr_t)io->n * (uintptr_t)io->F * 4u;
    const auto overlap = [](const void *p, uintptr_t pn, const void *q, uintptr_t qn) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
        return a < b + qn && b < a + pn;
    };
    if (overlap(io->dst, wbytes, io->src, wbytes)) return bad("dst overlaps src (the push is out of place: ping-pong two buffers)");
    if (overlap(io->dst, wbytes, io->fresh, fbytes)) return bad("dst overlaps fresh");
    WindowArgs a{};
    a.fresh = reinterpret_cast<const uint32_t *>(io->fresh);
    a.done = io->done;
    a.truncated = io->truncated;
    a.src = reinterpret_cast<const uint32_t *>(io->src);
    a.dst = reinterpret_cast<uint32_t *>(io->dst);
    a.T = io->T;
    a.F = io->F;
    a.n = io->n;
    HIP_TRY(window_push_launch(a, static_cast<hipStream_t>(stream)));
    return SUSNET_OK;
}
