// susnet_host.h -- what every host-side translation unit of the C ABI shares (susnet_capi*.hip; the launchers of inst_qnet_dense.hip and
// inst_mlp_train.hip take the LDS opt-in from here): the handle, the error conventions, the small helpers of the entry points, and the ONE
// statement of what a layer stack and a SpatialDQN are checked for (check_stack_*, check_spatial_net).
// Private to csrc/: the public interface is include/susnet.h.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "susnet_device.h"

struct susnet_env {
    susnet_config cfg;
    susnet::Consts c;
    susnet::State s;
    bool bound = false;
    bool float_exact = false;
    uint64_t ticks = 0; // steps taken (index of the production action stream)
    // test hooks, read ONCE at susnet_create (include/susnet.h SUSNET_OVERRIDE_*)
    bool force_generic = false;
    int ring_tile = 0;   // susnet_ring_append: environments of a wave's (ticks x envs) tile (8 / 16 / 32; 0: consecutive rows per wave)
    uint64_t launch_limit = (1ull << 31) - 1u, launch_limit_default = (1ull << 31) - 1u;
    int spec = 0; // pick_spec(): which compiled-in kernel family serves the handle (0 = generic)
    susnet_layout layout;
    uint64_t off_err, off_agent, off_job, off_jobdone, off_t, off_timer, off_flags, off_rng, off_msteps, off_mfix, off_msab,
        off_mkv, off_life, off_tickw, off_ep;
};

extern thread_local std::string g_err; // what susnet_last_error returns (defined in susnet_capi.hip)
inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
// (messages about a handle created under test hooks say so: a stray environment variable is then visible where it bites)
inline int fail(const susnet_env *env, int code, const std::string &msg) {
    std::string m = msg;
    if (env && env->layout.test_overrides) {
        m += " [handle created with";
        if (env->layout.test_overrides & SUSNET_OVERRIDE_FORCE_GENERIC) m += " SUSNET_FORCE_GENERIC";
        if (env->layout.test_overrides & SUSNET_OVERRIDE_EPW) m += " SUSNET_EPW";
        if (env->layout.test_overrides & SUSNET_OVERRIDE_TRAJ_MAX_BYTES) m += " SUSNET_TRAJ_MAX_BYTES";
        if (env->layout.test_overrides & SUSNET_OVERRIDE_RING_TILE) m += " SUSNET_RING_TILE";
        m += "]";
    }
    return fail(code, m);
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(SUSNET_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

inline uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

inline int check_bound(const susnet_env *env) {
    if (!env) return fail(SUSNET_E_INVALID, "null handle");
    if (!env->bound) return fail(SUSNET_E_STATE, "state blob not bound (susnet_bind_state)");
    return SUSNET_OK;
}
inline dim3 grid_for(const susnet_env *env) { return dim3((unsigned)((env->c.B + susnet::kBlock - 1) / susnet::kBlock)); }

// A kernel's dynamic-LDS ceiling (hipFuncAttributeMaxDynamicSharedMemorySize), raised once per device: a cheap host call, made on the first
// launch on a device and -- `opted` is the kernel's own flag array, one static per launch site -- never again, so after one eager step
// nothing is repeated inside a stream capture.  A device past the array is opted in on every call.
constexpr int kLdsOptInDevices = 64;
using LdsOptIn = std::atomic<bool>[kLdsOptInDevices];
inline hipError_t lds_opt_in(const void *kernel, int bytes, LdsOptIn &opted) {
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    const bool known = dev >= 0 && dev < kLdsOptInDevices;
    if (known && opted[dev].load(std::memory_order_acquire)) return hipSuccess;
    if (hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) return e;
    if (known) opted[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

// the Q-network entry points' own checks (susnet_capi_nets.hip), which the one-kernel tick and the fused learner share: the compiled-in
// feature layout of a component list on this handle (0 = none), and whether a layer stack fits QNet<ROW> (instantiated there for QRow1 /
// QRow3 / QRowC)
int qnet_feat(const susnet_env *env, const int32_t *comp, int32_t ncomp);
template <class ROW>
bool qnet_dims_ok(const int32_t *dims, int32_t n_dims);

// ---- a Linear / PReLU layer stack at an entry point (susnet_mlp_forward, susnet_spatial_forward's head, susnet_mlp_train_step): the ONE
// statement of what is checked, in which order and words, and of how an io's stack becomes a kernel's arguments ----
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; } // (float / int32 arrays: 4-byte)
// an entry point's refusal: SUSNET_E_INVALID, "<entry point>: <what>"
struct Refuse {
    const susnet_env *env;
    const char *entry;
    int operator()(const std::string &what) const { return fail(env, SUSNET_E_INVALID, std::string(entry) + ": " + what); }
};
// The dims of a stack are checked in three steps, in this order: n_dims, the caller's own rule for dims[0] (an `if` of its own, or
// check_feature_width), then the hidden widths and n_out.  `prefix` names the struct the fields sit in ("team[0]."), `layers` what n_dims counts
inline int check_stack_n_dims(const Refuse &bad, const std::string &prefix, int32_t n_dims, const char *layers = "1 .. 7 Linear layers") {
    if (n_dims < 2 || n_dims > 8) return bad(prefix + "n_dims = " + std::to_string(n_dims) + " (served: 2 .. 8, i.e. " + layers + ")");
    return SUSNET_OK;
}
inline int check_feature_width(const Refuse &bad, const std::string &prefix, int32_t F) { // (dims[0] of a stack that reads feature rows)
    if (F < 1 || F > SUSNET_MLP_MAX_F)
        return bad(prefix + "dims[0] = " + std::to_string(F) + " (F: 1 .. SUSNET_MLP_MAX_F = " + std::to_string(SUSNET_MLP_MAX_F) + ")");
    return SUSNET_OK;
}
inline int check_stack_dims(const Refuse &bad, const std::string &prefix, int32_t n_dims, const int32_t *dims, int max_hidden, int max_out) {
    const auto S = [](long long v) { return std::to_string(v); };
    const int nl = n_dims - 1;
    for (int l = 1; l < nl; l++)
        if (dims[l] < 1 || dims[l] > max_hidden) return bad(prefix + "dims[" + S(l) + "] = " + S(dims[l]) + " (hidden widths: 1 .. " + S(max_hidden) + ")");
    if (dims[nl] < 1 || dims[nl] > max_out) return bad(prefix + "dims[" + S(nl) + "] = " + S(dims[nl]) + " (n_out: 1 .. " + S(max_out) + ")");
    return SUSNET_OK;
}
// weight[l] / bias[l] of the nl layers, slope[l] of the nl - 1 activations between them: non-NULL and 4-byte aligned, layer by layer
inline int check_stack_ptrs(const Refuse &bad, const std::string &prefix, int nl, const float *const *weight, const float *const *bias,
                            const float *const *slope) {
    const auto at = [&](const char *field, int l) { return prefix + field + "[" + std::to_string(l) + "] is NULL or not 4-byte aligned"; };
    for (int l = 0; l < nl; l++) { // (the text is made where a pointer is refused: a served call allocates nothing here)
        if (!weight[l] || misaligned(weight[l])) return bad(at("weight", l));
        if (!bias[l] || misaligned(bias[l])) return bad(at("bias", l));
        if (l < nl - 1 && (!slope[l] || misaligned(slope[l]))) return bad(at("slope", l));
    }
    return SUSNET_OK;
}
// a checked io's stack (n_dims, dims, weight, bias, slope) into a kernel's argument struct (n_dims, d, W, B, A: DenseArgs, SpatialRnnArgs)
template <class ARGS, class IO>
inline void fill_stack(ARGS &a, const IO &io) {
    a.n_dims = io.n_dims;
    for (int l = 0; l < io.n_dims; l++) a.d[l] = io.dims[l];
    for (int l = 0; l < io.n_dims - 1; l++) a.W[l] = io.weight[l], a.B[l] = io.bias[l];
    for (int l = 0; l < io.n_dims - 2; l++) a.A[l] = io.slope[l];
}

// ---- a SpatialDQN at an entry point (susnet_spatial_forward; each enabled team of susnet_spatial_train_step): the ONE statement of its
// rules, their order -- T, N, C, n_conv, k, the conv layers, Fn, R, rnn_layers, rnn_hidden, then the head -- and their words.  `net_prefix`
// names the struct the spatial fields sit in ("net[0]."), `team_prefix` the one with the head's n_dims / dims ("team[0]."); NET is a
// susnet_spatial_net or the forward's susnet_spatial_io, which holds the same fields and the head inline (both prefixes empty) ----
struct SpatialGeom { // what every caller derives from a checked net, per activation level 0 .. n_conv
    int32_t size[SUSNET_SPATIAL_MAX_CONV + 1], ch[SUSNET_SPATIAL_MAX_CONV + 1], sz[SUSNET_SPATIAL_MAX_CONV + 1]; // image size, channels, floats (ch * size^2)
    int32_t Rc, R; // the RNN's input width R = Rc + Fn; its convolution columns
};
template <class NET>
inline int check_spatial_net(const Refuse &bad, const std::string &net_prefix, const std::string &team_prefix, const NET &sn, int32_t n_dims,
                             const int32_t *dims, int max_hidden, int max_out, SpatialGeom &g) {
    const auto S = [](long long v) { return std::to_string(v); };
    const auto range = [&](const std::string &field, long long v, long long lo, long long hi) {
        return net_prefix + field + " = " + S(v) + " (served: " + S(lo) + " .. " + S(hi) + ")";
    };
    if (sn.T < 1 || sn.T > SUSNET_SPATIAL_MAX_T) return bad(range("T", sn.T, 1, SUSNET_SPATIAL_MAX_T));
    if (sn.N < 1 || sn.N > SUSNET_SPATIAL_MAX_N) return bad(range("N", sn.N, 1, SUSNET_SPATIAL_MAX_N));
    if (sn.C < 1 || sn.C > SUSNET_SPATIAL_MAX_C) return bad(range("C", sn.C, 1, SUSNET_SPATIAL_MAX_C));
    if (sn.n_conv < 1 || sn.n_conv > SUSNET_SPATIAL_MAX_CONV) return bad(range("n_conv", sn.n_conv, 1, SUSNET_SPATIAL_MAX_CONV));
    if (sn.k != 1 && sn.k != 3 && sn.k != 5) return bad(net_prefix + "k = " + S(sn.k) + " (served: one square kernel size of 1, 3 or 5)");
    g = SpatialGeom{};
    g.size[0] = sn.N, g.ch[0] = sn.C, g.sz[0] = sn.C * sn.N * sn.N;
    for (int l = 0; l < sn.n_conv; l++) {
        const std::string at = "[" + S(l) + "]";
        if (sn.conv_out[l] < 1 || sn.conv_out[l] > 32) return bad(range("conv_out" + at, sn.conv_out[l], 1, 32));
        if (sn.conv_stride[l] < 1 || sn.conv_stride[l] > 4) return bad(range("conv_stride" + at, sn.conv_stride[l], 1, 4));
        if (sn.conv_padding[l] < 0 || sn.conv_padding[l] > 8) return bad(range("conv_padding" + at, sn.conv_padding[l], 0, 8));
        if (sn.conv_dilation[l] < 1 || sn.conv_dilation[l] > 4) return bad(range("conv_dilation" + at, sn.conv_dilation[l], 1, 4));
        const int span = g.size[l] + 2 * sn.conv_padding[l] - sn.conv_dilation[l] * (sn.k - 1) - 1;
        if (span < 0) return bad(net_prefix + "conv layer " + S(l) + ": output size < 1 (input " + S(g.size[l]) + ", k " + S(sn.k) + ", conv_padding" + at +
                                 " " + S(sn.conv_padding[l]) + ", conv_dilation" + at + " " + S(sn.conv_dilation[l]) + ")");
        g.size[l + 1] = span / sn.conv_stride[l] + 1;
        g.ch[l + 1] = sn.conv_out[l];
        g.sz[l + 1] = g.ch[l + 1] * g.size[l + 1] * g.size[l + 1];
    }
    if (sn.Fn < 0) return bad(net_prefix + "Fn = " + S(sn.Fn) + " (at least 0)");
    const long long R = (long long)g.sz[sn.n_conv] + sn.Fn;
    if (R > SUSNET_SPATIAL_MAX_R)
        return bad(net_prefix + "R = conv_out * H_out^2 + Fn = " + S(R) + " (the RNN's input width: at most SUSNET_SPATIAL_MAX_R = " + S(SUSNET_SPATIAL_MAX_R) + ")");
    g.Rc = g.sz[sn.n_conv], g.R = (int32_t)R;
    if (sn.rnn_layers < 1 || sn.rnn_layers > SUSNET_SPATIAL_MAX_RNN_LAYERS) return bad(range("rnn_layers", sn.rnn_layers, 1, SUSNET_SPATIAL_MAX_RNN_LAYERS));
    if (sn.rnn_hidden < 1 || sn.rnn_hidden > max_hidden) return bad(range("rnn_hidden", sn.rnn_hidden, 1, max_hidden));
    if (int rc = check_stack_n_dims(bad, team_prefix, n_dims, "a head of 1 .. 7 Linear layers")) return rc;
    if (dims[0] != sn.rnn_hidden)
        return bad(team_prefix + "dims[0] = " + S(dims[0]) + " (the head reads the hidden state: " + net_prefix + "rnn_hidden = " + S(sn.rnn_hidden) + ")");
    return check_stack_dims(bad, team_prefix, n_dims, dims, max_hidden, max_out);
}
