// susnet_capi_ring.hip -- susnet_ring_append: a rollout's trajectory into the replay ring's tensors (kernels and entry point).
// Scheduled like susnet_capi.hip (build_hip.flags_for): these kernels run many waves per SIMD and live on occupancy.
#include "susnet_host.h"
#include "susnet_obs.h" // wave_lds_fence

using namespace susnet;

struct RingArgs {
    susnet_ring_io io;
    int64_t B, n0, n1; // envs; first / one-past-last transition (n = tick * B + env) this launch writes
    int32_t A, S, n_imp;
    int32_t rows_per_wave; // 64, or fewer when 64 rows of 2 x trajectory_size x S bytes would not fit the LDS images
    int32_t tile_log2e;    // k_ring_append_tile: log2 of the tile's environments (3: 8 ticks x 8 envs)
    int32_t n0_b;            // n0 = n0_t * B + n0_b; pos_n0 = ring position of transition n0
    int64_t n0_t, pos_n0;
    // the trajectory as PACKED RECORDS (io.record; whole records only: the 1v1 kernels), wave-uniform: record size (0 = separate
    // tensors) and field offsets; rec_packed: actions and flags share one byte (SUSNET_RECORD_COMPACT)
    int32_t rec_bytes, rec_obs, rec_act, rec_rew, rec_done, rec_trunc, rec_packed;
};
// the trajectory's fields at (tick u, env b), from the separate tensors or from the records -- a compile-time choice (REC): as a run-time
// one every access carried a uniform branch and both address forms, and the append of the small 1v1 rows ran at 81 us instead of 56
__device__ __forceinline__ const uint8_t *ring_rec(const RingArgs &r, int64_t u, int64_t b) { return r.io.record + ((size_t)u * r.B + b) * (size_t)r.rec_bytes; }
template <bool REC>
__device__ __forceinline__ uint32_t ring_done(const RingArgs &r, int64_t u, int64_t b) {
    if constexpr (REC) return r.rec_packed ? (ring_rec(r, u, b)[r.rec_done] >> 6) & 1u : (uint32_t)ring_rec(r, u, b)[r.rec_done];
    else return r.io.done[u * r.B + b];
}
template <bool REC>
__device__ __forceinline__ uint32_t ring_trunc(const RingArgs &r, int64_t u, int64_t b) {
    if constexpr (REC) return r.rec_packed ? (uint32_t)(ring_rec(r, u, b)[r.rec_trunc] >> 7) : (uint32_t)ring_rec(r, u, b)[r.rec_trunc];
    else return r.io.truncated[u * r.B + b];
}
template <bool REC>
__device__ __forceinline__ uint32_t ring_action(const RingArgs &r, int64_t t, int64_t b, int i) {
    if constexpr (REC) return r.rec_packed ? (ring_rec(r, t, b)[r.rec_act] >> (3 * i)) & 7u : (uint32_t)ring_rec(r, t, b)[r.rec_act + i];
    else return r.io.actions[((size_t)t * r.B + b) * r.A + i];
}
template <bool REC>
__device__ __forceinline__ float ring_reward(const RingArgs &r, int64_t t, int64_t b, int i) {
    if constexpr (REC) return reinterpret_cast<const float *>(ring_rec(r, t, b) + r.rec_rew)[i];
    else return r.io.rewards[((size_t)t * r.B + b) * r.A + i];
}
// the flattened state an env's window holds at virtual tick u (= the state after tick u; u < 0: the carried-in window)
template <bool REC>
__device__ __forceinline__ const uint8_t *ring_state(const RingArgs &r, int64_t u, int64_t b) {
    const int Tw = r.io.trajectory_size;
    if (u < 0) return r.io.window + ((size_t)b * Tw + (size_t)(Tw + u < 0 ? 0 : Tw + u)) * r.S; // window[Tw - 1] = state before tick 0
    if constexpr (REC) return ring_rec(r, u, b) + r.rec_obs;
    else return r.io.obs + ((size_t)u * r.B + b) * r.S;
}
// One wave per 64 consecutive transitions (32 / 16 / 8 for long windows: RingArgs::rows_per_wave).
// Lane r gathers what its row needs into flat images in LDS, laid out exactly as the wave's 64 rows lie in each ring tensor (row-major;
// `states` and `next_states`: Tw * S bytes per row, the Tw - 1 shared states written to both; actions, rewards, done, imposters
// likewise), and the wave then writes every tensor as ONE linear range: 16 bytes per lane and step, no index arithmetic.  (One image of
// Tw + 1 states per row, read at offsets 0 and S, needs a quarter less LDS but its reads are unaligned dwords: measured 2.1 / 3.4 TB/s
// against 3.0 / 4.2 on the 1v1 and 1v2 shapes.)
// Two things made the first version slow (3.1-3.5 TB/s, 82 % of the wave cycles waiting): every element index was divided by Tw * S to
// find its row, and each lane stored its row's small tensors between its loads -- stores the loads behind them had to wait for
// (may-alias), one memory round trip per element.  Now a lane only LOADS in the gather phase (flags first, unrolled without an early
// exit; then rows, actions, rewards, roles) and all global stores happen after it.
constexpr int kRingFlagsUnroll = 8;
constexpr int kRingGroup = 3, kRingChunk = 8; // source states per load group; dwords of a state per load group
template <bool REC>
__global__ __launch_bounds__(64) void k_ring_append(RingArgs r) {
    extern __shared__ uint32_t smem[];
    const int lane = threadIdx.x, Tw = r.io.trajectory_size, S = r.S, A = r.A, NI = r.n_imp;
    const int R = r.rows_per_wave;
    const int TS = Tw * S;
    const int img = (R * TS + 15) & ~15; // bytes of one state image (padded: the vector loops read up to 3 bytes past the last row)
    uint8_t *st_img = reinterpret_cast<uint8_t *>(smem), *nx_img = st_img + img;
    float *rew_img = reinterpret_cast<float *>(nx_img + img);        // [R][A]
    uint8_t *act_img = reinterpret_cast<uint8_t *>(rew_img + R * A); // [R][A] (+ pad)
    uint8_t *done_img = act_img + ((R * A + 15) & ~15);              // [R]
    int16_t *imp_img = reinterpret_cast<int16_t *>(done_img + 64);   // [R][NI]
    // (tick, env) of the lane's transition n = n0 + rel + lane without a 64-bit division per lane: the host supplies n0's, the rest is
    // 32-bit (rel + B < 2^32: checked there)
    const uint32_t rel = (uint32_t)blockIdx.x * (uint32_t)R;
    const int64_t n_first = r.n0 + (int64_t)rel;
    const int rows = (int)((r.n1 - n_first) < R ? (r.n1 - n_first) : R);
    if (lane < rows) {
        const uint32_t x = rel + (uint32_t)r.n0_b + (uint32_t)lane, tq = x / (uint32_t)r.B;
        const int64_t t = r.n0_t + (int64_t)tq, b = (int64_t)(x - tq * (uint32_t)r.B);
        // most recent episode boundary before tick t within the window's reach (the episode's first state is obs[e]); all flag
        // loads are independent of each other
        int64_t e = -(1ll << 62);
        if (Tw <= kRingFlagsUnroll) {
            uint32_t fd[kRingFlagsUnroll], ft[kRingFlagsUnroll];
#pragma unroll
            for (int k = 1; k <= kRingFlagsUnroll; k++) { // every lane loads (tick clamped): no per-lane branch, no wait between the loads
                const int64_t u = t - k < 0 ? 0 : t - k;
                const bool want = k <= Tw; // (wave-uniform)
                fd[k - 1] = want ? ring_done<REC>(r, u, b) : 0u;
                ft[k - 1] = want ? ring_trunc<REC>(r, u, b) : 0u;
            }
#pragma unroll
            for (int k = kRingFlagsUnroll; k >= 1; k--)
                if ((fd[k - 1] | ft[k - 1]) != 0u && t - k >= 0) e = t - k; // (descending k: the most recent boundary wins)
        } else {
            for (int64_t u = t - 1; u >= 0 && u > t - 1 - Tw; u--)
                if (ring_done<REC>(r, u, b) | ring_trunc<REC>(r, u, b)) { e = u; break; }
        }
        const uint32_t dn = ring_done<REC>(r, t, b), tr = ring_trunc<REC>(r, t, b);
        const uint32_t role_bits = r.io.roles ? (uint32_t)r.io.roles[t * r.B + b] : ((1u << NI) - 1u);
        uint8_t *my_st = st_img + (size_t)lane * TS, *my_nx = nx_img + (size_t)lane * TS;
        // The row needs Tw + 1 source states (replay_memory.py:108-113, 122-127): the window's Tw states -> states[k], and shifted by one
        // -> next_states[k - 1]; the state after the tick (the terminal observation where the episode ended) -> next_states[Tw - 1].  A
        // state = S consecutive bytes at an arbitrary address, fetched as UNALIGNED dwords (gfx950 serves them, global and LDS alike) + a
        // byte tail.  All loads of a group of kRingGroup states are issued before the first LDS store: one memory round trip per group,
        // not one per dword (the rolled load -> store loop this replaces made 18 dependent round trips per row and left the kernel
        // latency-bound at 3.7 TB/s).
        const uint8_t *nxt = (dn | tr) ? r.io.term_obs + ((size_t)t * r.B + b) * S : ring_state<REC>(r, t, b);
        auto source = [&](int k) -> const uint8_t * {
            if (k >= Tw) return nxt;
            int64_t u = t - Tw + k;
            if (u < e) u = e;
            return ring_state<REC>(r, u, b);
        };
        for (int k0 = 0; k0 <= Tw; k0 += kRingGroup) {
            for (int c0 = 0; c0 < S; c0 += 4 * kRingChunk) {
                uint32_t v[kRingGroup][kRingChunk];
                uint8_t tail[kRingGroup][3];
#pragma unroll
                for (int g = 0; g < kRingGroup; g++) {
                    if (k0 + g > Tw) break; // (wave-uniform)
                    const uint8_t *src = source(k0 + g) + c0;
#pragma unroll
                    for (int q = 0; q < kRingChunk; q++)
                        if (c0 + 4 * q + 4 <= S) __builtin_memcpy(&v[g][q], src + 4 * q, 4);
                    if (S - c0 < 4 * kRingChunk) { // the row ends in this chunk: its last S % 4 bytes
                        const int f0 = (S - c0) & ~3;
#pragma unroll
                        for (int q = 0; q < 3; q++)
                            if (f0 + q < S - c0) tail[g][q] = src[f0 + q];
                    }
                }
#pragma unroll
                for (int g = 0; g < kRingGroup; g++) {
                    const int k = k0 + g;
                    if (k > Tw) break;
                    uint8_t *d0 = k < Tw ? my_st + k * S + c0 : nullptr, *d1 = k > 0 ? my_nx + (k - 1) * S + c0 : nullptr;
#pragma unroll
                    for (int q = 0; q < kRingChunk; q++)
                        if (c0 + 4 * q + 4 <= S) {
                            if (d0) __builtin_memcpy(d0 + 4 * q, &v[g][q], 4);
                            if (d1) __builtin_memcpy(d1 + 4 * q, &v[g][q], 4);
                        }
                    if (S - c0 < 4 * kRingChunk) {
                        const int f0 = (S - c0) & ~3;
#pragma unroll
                        for (int q = 0; q < 3; q++)
                            if (f0 + q < S - c0) {
                                if (d0) d0[f0 + q] = tail[g][q];
                                if (d1) d1[f0 + q] = tail[g][q];
                            }
                    }
                }
            }
        }
        for (int i0 = 0; i0 < A; i0 += 8) { // (loads of eight agents in flight, then their LDS stores)
            uint8_t av[8];
            float rv[8];
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (i0 + q < A) {
                    av[q] = (uint8_t)ring_action<REC>(r, t, b, i0 + q);
                    rv[q] = ring_reward<REC>(r, t, b, i0 + q);
                }
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (i0 + q < A) {
                    act_img[lane * A + i0 + q] = av[q];
                    rew_img[lane * A + i0 + q] = rv[q];
                }
        }
        done_img[lane] = dn ? 1 : 0; // replay_memory.py:131: done, not truncation
        uint32_t m = role_bits;
        for (int k = 0; k < NI; k++) { // ascending agent indices
            const int i = __ffs((int)m) - 1;
            imp_img[lane * NI + k] = (int16_t)(i < 0 ? 0 : i);
            m &= m - 1u;
        }
    }
    wave_lds_fence();
    // ring position of row 0 of this wave; rows are consecutive positions modulo max_size
    int64_t pos0 = r.pos_n0 + (int64_t)rel; // (pos_n0 = (idx + n0) % max_size from the host; rel < max_size)
    if (pos0 >= r.io.max_size) pos0 -= r.io.max_size;
    const int total = rows * TS;
    if (__builtin_expect(pos0 + rows <= r.io.max_size, 1)) { // no wrap inside the wave: every output is ONE contiguous range
        float *out_s = r.io.states + (size_t)pos0 * TS, *out_n = r.io.next_states + (size_t)pos0 * TS;
        if ((((size_t)pos0 * TS) & 3u) == 0) { // 16-byte aligned ranges: four elements per lane and step
            const uint32_t *s4 = reinterpret_cast<const uint32_t *>(st_img), *n4 = reinterpret_cast<const uint32_t *>(nx_img);
            for (int g = 4 * lane; g < total; g += 256) {
                const uint32_t a = s4[g >> 2], c = n4[g >> 2];
                const float4 fa = make_float4((float)(a & 0xffu), (float)((a >> 8) & 0xffu), (float)((a >> 16) & 0xffu), (float)(a >> 24));
                const float4 fc = make_float4((float)(c & 0xffu), (float)((c >> 8) & 0xffu), (float)((c >> 16) & 0xffu), (float)(c >> 24));
                if (g + 4 <= total) {
                    *reinterpret_cast<float4 *>(out_s + g) = fa;
                    *reinterpret_cast<float4 *>(out_n + g) = fc;
                } else { // the range's last, partial group
                    const float va[4] = {fa.x, fa.y, fa.z, fa.w}, vc[4] = {fc.x, fc.y, fc.z, fc.w};
                    for (int q = 0; q < total - g; q++) { out_s[g + q] = va[q]; out_n[g + q] = vc[q]; }
                }
            }
        } else {
            for (int g = lane; g < total; g += 64) {
                out_s[g] = (float)st_img[g];
                out_n[g] = (float)nx_img[g];
            }
        }
        int64_t *out_a = r.io.ring_actions + (size_t)pos0 * A;
        float *out_r = r.io.ring_rewards + (size_t)pos0 * A;
        for (int g = lane; g < rows * A; g += 64) {
            out_a[g] = (int64_t)act_img[g];
            out_r[g] = rew_img[g];
        }
        if (lane < rows) r.io.ring_dones[pos0 + lane] = done_img[lane];
        for (int g = lane; g < rows * NI; g += 64) r.io.ring_imposters[(size_t)pos0 * NI + g] = imp_img[g];
    } else { // the ring wraps inside this wave's rows (once per trip round the ring): element by element
        for (int g = lane; g < total; g += 64) {
            const int row = g / TS, k = g - row * TS;
            int64_t p = pos0 + row;
            if (p >= r.io.max_size) p -= r.io.max_size;
            r.io.states[(size_t)p * TS + k] = (float)st_img[g];
            r.io.next_states[(size_t)p * TS + k] = (float)nx_img[g];
        }
        if (lane < rows) {
            int64_t p = pos0 + lane;
            if (p >= r.io.max_size) p -= r.io.max_size;
            for (int i = 0; i < A; i++) {
                r.io.ring_actions[p * A + i] = (int64_t)act_img[lane * A + i];
                r.io.ring_rewards[p * A + i] = rew_img[lane * A + i];
            }
            r.io.ring_dones[p] = done_img[lane];
            for (int k = 0; k < NI; k++) r.io.ring_imposters[p * NI + k] = imp_img[lane * NI + k];
        }
    }
}
// The same rows from a TILE per wave: TT consecutive ticks x TE consecutive environments (TT * TE = 64; lane = dt * TE + db).  A row needs
// the Tw + 1 states around its tick (replay_memory.py:108-113, 122-127) and in the kernel above every lane fetches all of them itself:
// each state of the trajectory is read by Tw + 1 waves.  Here the wave fetches the (TT + Tw) x TE states its tile touches ONCE into an
// LDS image (one state per lane + Tw * TE states ahead of the tile + the terminal states where an episode ended) and every lane then
// assembles its row from that image: (TT + Tw) / TT reads per state instead of Tw + 1.  The rows of one tick are TE consecutive ring
// positions, so the wave writes TT contiguous runs per tensor; run bases live in a small LDS table and the store loop walks all runs as
// one flattened index space (run = index / groups-per-run by a multiply), 16 bytes per lane and step as above.
struct RingRun {
    int64_t pos;      // ring position of the run's first row
    int32_t first, n; // first lane-row of the run in the images (dt * TE + lo); rows (0: nothing to write; < 0: -n rows, the ring wraps inside)
};
__device__ __forceinline__ void ring_copy_state(uint8_t *d0, uint8_t *d1, const uint8_t *src, int S) {
    int c = 0;
    for (; c + 16 <= S; c += 16) {
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) __builtin_memcpy(&v[q], src + c + 4 * q, 4);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (d0) __builtin_memcpy(d0 + c + 4 * q, &v[q], 4);
            if (d1) __builtin_memcpy(d1 + c + 4 * q, &v[q], 4);
        }
    }
    for (; c + 4 <= S; c += 4) {
        uint32_t v;
        __builtin_memcpy(&v, src + c, 4);
        if (d0) __builtin_memcpy(d0 + c, &v, 4);
        if (d1) __builtin_memcpy(d1 + c, &v, 4);
    }
    for (; c < S; c++) {
        const uint8_t v = src[c];
        if (d0) d0[c] = v;
        if (d1) d1[c] = v;
    }
}
template <bool REC>
__global__ __launch_bounds__(64) void k_ring_append_tile(RingArgs r) {
    extern __shared__ uint32_t smem[];
    const int lane = threadIdx.x, Tw = r.io.trajectory_size, S = r.S, A = r.A, NI = r.n_imp;
    const int le = r.tile_log2e, TE = 1 << le, TT = 64 >> le;
    const int64_t tiles_b = (r.B + TE - 1) >> le;
    const int64_t tile_t = (int64_t)blockIdx.x / tiles_b, tile_b = (int64_t)blockIdx.x - tile_t * tiles_b;
    const int64_t t_first = r.n0 / r.B; // first tick with a row to write
    const int64_t t0 = t_first + tile_t * TT, b0 = tile_b << le;
    const int dt = lane >> le, db = lane & (TE - 1);
    const int64_t t = t0 + dt, b = b0 + db;
    const bool live = t < r.io.n_ticks && b < r.B; // the lane's (tick, env) exists (its row is written only if t * B + b >= n0)
    const int TS = Tw * S;
    // LDS: [source states (TT + Tw) x TE][their episode-end flags][states image 64 x TS][next_states image][rewards][actions][done][imposters][runs]
    const int n_src = (TT + Tw) * TE;
    uint8_t *src_img = reinterpret_cast<uint8_t *>(smem);
    uint8_t *flg_img = src_img + ((n_src * S + 15) & ~15);
    uint8_t *st_img = flg_img + ((n_src + 15) & ~15);
    const int img = (64 * TS + 15) & ~15;
    uint8_t *nx_img = st_img + img;
    float *rew_img = reinterpret_cast<float *>(nx_img + img);
    uint8_t *act_img = reinterpret_cast<uint8_t *>(rew_img + 64 * A);
    uint8_t *done_img = act_img + ((64 * A + 15) & ~15);
    int16_t *imp_img = reinterpret_cast<int16_t *>(done_img + 64);
    RingRun *runs = reinterpret_cast<RingRun *>(reinterpret_cast<uint8_t *>(imp_img) + ((64 * NI * 2 + 15) & ~15));
    uint8_t *my_st = st_img + (size_t)lane * TS, *my_nx = nx_img + (size_t)lane * TS;

    // ---- phase A: every global load of the tile, then the LDS stores
    uint32_t dn = 0, tr = 0;
    if (live) { dn = ring_done<REC>(r, t, b); tr = ring_trunc<REC>(r, t, b); }
    const bool ended = (dn | tr) != 0u;
    // the Tw ticks ahead of the tile: lane = du * TE + db' for du < Tw (Tw * TE <= 64: checked on the host)
    const int du = lane >> le;
    const int64_t u_pre = t0 - Tw + du;
    const bool pre = du < Tw && b < r.B;
    uint32_t pre_flag = 0;
    if (pre && u_pre >= 0) pre_flag = ring_done<REC>(r, u_pre, b) | ring_trunc<REC>(r, u_pre, b);
    const uint8_t *sp[3] = {live ? ring_state<REC>(r, t, b) : nullptr, pre ? ring_state<REC>(r, u_pre, b) : nullptr,
                            live && ended ? r.io.term_obs + ((size_t)t * r.B + b) * S : nullptr};
    uint8_t *own_slot = src_img + (size_t)((dt + Tw) * TE + db) * S, *pre_slot = src_img + (size_t)(du * TE + db) * S, *last = my_nx + (size_t)(Tw - 1) * S;
    for (int c0 = 0; c0 < S; c0 += 4 * kRingChunk) {
        uint32_t v[3][kRingChunk];
        uint8_t tail[3][3];
#pragma unroll
        for (int g = 0; g < 3; g++) {
            if (sp[g] == nullptr) continue;
            const uint8_t *src = sp[g] + c0;
#pragma unroll
            for (int q = 0; q < kRingChunk; q++)
                if (c0 + 4 * q + 4 <= S) __builtin_memcpy(&v[g][q], src + 4 * q, 4);
            if (S - c0 < 4 * kRingChunk) {
                const int f0 = (S - c0) & ~3;
#pragma unroll
                for (int q = 0; q < 3; q++)
                    if (f0 + q < S - c0) tail[g][q] = src[f0 + q];
            }
        }
#pragma unroll
        for (int g = 0; g < 3; g++) {
            if (sp[g] == nullptr) continue;
            // own state -> its source slot, and the row's last next-state unless the episode ended (then the terminal state is)
            uint8_t *d0 = g == 0 ? own_slot + c0 : g == 1 ? pre_slot + c0 : last + c0;
            uint8_t *d1 = g == 0 && !ended ? last + c0 : nullptr;
#pragma unroll
            for (int q = 0; q < kRingChunk; q++)
                if (c0 + 4 * q + 4 <= S) {
                    __builtin_memcpy(d0 + 4 * q, &v[g][q], 4);
                    if (d1) __builtin_memcpy(d1 + 4 * q, &v[g][q], 4);
                }
            if (S - c0 < 4 * kRingChunk) {
                const int f0 = (S - c0) & ~3;
#pragma unroll
                for (int q = 0; q < 3; q++)
                    if (f0 + q < S - c0) {
                        d0[f0 + q] = tail[g][q];
                        if (d1) d1[f0 + q] = tail[g][q];
                    }
            }
        }
    }
    if (live) {
        const uint32_t role_bits = r.io.roles ? (uint32_t)r.io.roles[t * r.B + b] : ((1u << NI) - 1u);
        for (int i0 = 0; i0 < A; i0 += 8) {
            uint8_t av[8];
            float rv[8];
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (i0 + q < A) {
                    av[q] = (uint8_t)ring_action<REC>(r, t, b, i0 + q);
                    rv[q] = ring_reward<REC>(r, t, b, i0 + q);
                }
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (i0 + q < A) {
                    act_img[lane * A + i0 + q] = av[q];
                    rew_img[lane * A + i0 + q] = rv[q];
                }
        }
        done_img[lane] = dn ? 1 : 0; // replay_memory.py:131: done, not truncation
        uint32_t m = role_bits;
        for (int k = 0; k < NI; k++) { // ascending agent indices
            const int i = __ffs((int)m) - 1;
            imp_img[lane * NI + k] = (int16_t)(i < 0 ? 0 : i);
            m &= m - 1u;
        }
    }
    flg_img[(dt + Tw) * TE + db] = ended ? 1 : 0;
    if (du < Tw) flg_img[du * TE + db] = pre_flag ? 1 : 0;
    if (lane < TT) { // the runs: tick t0 + lane, rows [lo, hi) of the tile's TE environments
        const int64_t tt = t0 + lane;
        RingRun run = {0, 0, 0};
        if (tt < r.io.n_ticks) {
            const int64_t nb = tt * r.B + b0; // transition index of the run's first environment
            const int lo = nb >= r.n0 ? 0 : (r.n0 - nb >= TE ? TE : (int)(r.n0 - nb));
            const int hi = r.B - b0 >= TE ? TE : (int)(r.B - b0);
            if (hi > lo) {
                run.pos = (r.io.idx + nb + lo) % r.io.max_size;
                run.first = lane * TE + lo;
                run.n = run.pos + (hi - lo) <= r.io.max_size ? hi - lo : -(hi - lo);
            }
        }
        runs[lane] = run;
    }
    wave_lds_fence();

    // ---- phase B: the row's window from the source image (states[k] and, shifted by one, next_states[k - 1])
    if (live) {
        int64_t e = -(1ll << 62); // most recent episode boundary before tick t within the window's reach
        for (int k = Tw; k >= 1; k--)
            if (flg_img[(dt + Tw - k) * TE + db] != 0 && t - k >= 0) e = t - k;
        for (int k = 0; k < Tw; k++) {
            int64_t u = t - Tw + k;
            if (u < e) u = e;
            const uint8_t *src = src_img + (size_t)((int)(u - t0 + Tw) * TE + db) * S;
            ring_copy_state(my_st + (size_t)k * S, k > 0 ? my_nx + (size_t)(k - 1) * S : nullptr, src, S);
        }
    }
    wave_lds_fence();

    // ---- phase C: TT contiguous runs per tensor
    const uint32_t run_elems = (uint32_t)(TE * TS); // floats of a full run
    bool fast = true;                              // every run: no wrap inside, 16-byte aligned start, whole groups of four floats
#pragma unroll 1
    for (int q = 0; q < TT; q++) {
        const RingRun run = runs[q];
        if (run.n < 0 || ((((size_t)run.pos * TS) | (size_t)((run.first & (TE - 1)) * TS) | (size_t)(run.n > 0 ? run.n * TS : 0)) & 3u) != 0) fast = false;
    }
    if (__builtin_expect(fast, 1)) {
        const uint32_t gpr = run_elems >> 2; // float4 groups of a full run (a shorter run: the groups past its end are skipped)
        const uint32_t magic = 0xffffffffu / gpr + 1u;
        const uint32_t total = gpr * (uint32_t)TT;
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>(st_img), *n4 = reinterpret_cast<const uint32_t *>(nx_img);
        for (uint32_t g = lane; g < total; g += 64) {
            const uint32_t q = __umulhi(g, magic), w = g - q * gpr;
            const RingRun run = runs[q];
            if ((int)(4 * w) >= run.n * TS) continue;
            const uint32_t at = (uint32_t)run.first * (uint32_t)TS + 4 * w; // byte offset into the images (a multiple of 4: checked above)
            const uint32_t a = s4[at >> 2], c = n4[at >> 2];
            const float4 fa = make_float4((float)(a & 0xffu), (float)((a >> 8) & 0xffu), (float)((a >> 16) & 0xffu), (float)(a >> 24));
            const float4 fc = make_float4((float)(c & 0xffu), (float)((c >> 8) & 0xffu), (float)((c >> 16) & 0xffu), (float)(c >> 24));
            const size_t o = (size_t)run.pos * TS + 4 * w;
            *reinterpret_cast<float4 *>(r.io.states + o) = fa;
            *reinterpret_cast<float4 *>(r.io.next_states + o) = fc;
        }
    } else { // a run that wraps round the ring's end or starts off a 16-byte boundary: element by element
        for (int q = 0; q < TT; q++) {
            const RingRun run = runs[q];
            const int n = run.n < 0 ? -run.n : run.n;
            for (int g = lane; g < n * TS; g += 64) {
                const int row = g / TS, k = g - row * TS;
                int64_t p = run.pos + row;
                if (p >= r.io.max_size) p -= r.io.max_size;
                r.io.states[(size_t)p * TS + k] = (float)st_img[(size_t)run.first * TS + g];
                r.io.next_states[(size_t)p * TS + k] = (float)nx_img[(size_t)run.first * TS + g];
            }
        }
    }
    // the small tensors: lane-row l of the images is row l - run.first of run l / TE
    {
        const RingRun run = runs[dt];
        const int n = run.n < 0 ? -run.n : run.n;
        const int row = lane - run.first;
        if (row >= 0 && row < n) {
            int64_t p = run.pos + row;
            if (p >= r.io.max_size) p -= r.io.max_size;
            r.io.ring_dones[p] = done_img[lane];
            for (int k = 0; k < NI; k++) r.io.ring_imposters[p * NI + k] = imp_img[lane * NI + k];
        }
        const uint32_t magic_a = 0xffffffffu / (uint32_t)A + 1u;
        for (uint32_t g = lane; g < 64u * (uint32_t)A; g += 64) { // consecutive lanes: consecutive elements of a run
            const uint32_t l = __umulhi(g, magic_a), i = g - l * (uint32_t)A;
            const RingRun rl = runs[l >> le];
            const int nl = rl.n < 0 ? -rl.n : rl.n, rw = (int)l - rl.first;
            if (rw < 0 || rw >= nl) continue;
            int64_t p = rl.pos + rw;
            if (p >= r.io.max_size) p -= r.io.max_size;
            r.io.ring_actions[p * A + i] = (int64_t)act_img[g];
            r.io.ring_rewards[p * A + i] = rew_img[g];
        }
    }
}
// the carried window of every env after the launch: the window before the tick that follows the last one
template <bool REC>
__global__ __launch_bounds__(64) void k_ring_window(RingArgs r) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= r.B) return;
    const int Tw = r.io.trajectory_size, S = r.S;
    const int64_t t = r.io.n_ticks;
    int64_t e = -(1ll << 62);
    for (int64_t u = t - 1; u >= 0 && u > t - 1 - Tw; u--)
        if (ring_done<REC>(r, u, b) | ring_trunc<REC>(r, u, b)) { e = u; break; }
    // in place, slots ascending: slot k of the new window comes from obs, or (launches shorter than the window) from slot
    // k + t > k of the old one, which has not been overwritten yet
    // (a group's loads are all issued before its first store, as in k_ring_append: a slot read from the old window lies above every slot
    // written so far)
    uint8_t *dst = r.io.window + (size_t)b * Tw * S;
    for (int k0 = 0; k0 < Tw; k0 += kRingGroup) {
        for (int c0 = 0; c0 < S; c0 += 4 * kRingChunk) {
            uint32_t v[kRingGroup][kRingChunk];
            uint8_t tail[kRingGroup][3];
#pragma unroll
            for (int g = 0; g < kRingGroup; g++) {
                if (k0 + g >= Tw) break;
                int64_t u = t - Tw + k0 + g;
                if (u < e) u = e;
                const uint8_t *src = ring_state<REC>(r, u, b) + c0;
#pragma unroll
                for (int q = 0; q < kRingChunk; q++)
                    if (c0 + 4 * q + 4 <= S) __builtin_memcpy(&v[g][q], src + 4 * q, 4);
                if (S - c0 < 4 * kRingChunk) {
                    const int f0 = (S - c0) & ~3;
#pragma unroll
                    for (int q = 0; q < 3; q++)
                        if (f0 + q < S - c0) tail[g][q] = src[f0 + q];
                }
            }
#pragma unroll
            for (int g = 0; g < kRingGroup; g++) {
                if (k0 + g >= Tw) break;
                uint8_t *d = dst + (k0 + g) * S + c0;
#pragma unroll
                for (int q = 0; q < kRingChunk; q++)
                    if (c0 + 4 * q + 4 <= S) __builtin_memcpy(d + 4 * q, &v[g][q], 4);
                if (S - c0 < 4 * kRingChunk) {
                    const int f0 = (S - c0) & ~3;
#pragma unroll
                    for (int q = 0; q < 3; q++)
                        if (f0 + q < S - c0) d[f0 + q] = tail[g][q];
                }
            }
        }
    }
}

extern "C" int susnet_ring_append(susnet_env *env, const susnet_ring_io *io, void *stream) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "null argument");
    if (io->n_ticks < 1 || io->trajectory_size < 1 || io->max_size < 1 || io->idx < 0 || io->idx >= io->max_size)
        return fail(SUSNET_E_INVALID, "susnet_ring_append: n_ticks, trajectory_size, max_size must be positive and 0 <= idx < max_size");
    const bool from_records = io->record != nullptr;
    if (from_records && (io->actions || io->rewards || io->done || io->truncated || io->obs))
        return fail(SUSNET_E_INVALID, "susnet_ring_append: record is an alternative to the separate trajectory tensors, not an addition");
    if ((!from_records && (!io->actions || !io->rewards || !io->done || !io->truncated || !io->obs)) || !io->term_obs || !io->window || !io->states ||
        !io->next_states || !io->ring_actions || !io->ring_rewards || !io->ring_dones || !io->ring_imposters)
        return fail(SUSNET_E_INVALID, "susnet_ring_append: null buffer");
    if (!io->roles && env->c.shuffle_imp) return fail(SUSNET_E_INVALID, "susnet_ring_append: roles are drawn per episode here (shuffle_imposter_index): pass roles");
    RingArgs r;
    r.io = *io;
    r.B = env->c.B;
    r.A = env->c.A;
    r.S = env->layout.obs_raw_size;
    r.n_imp = env->c.n_imp;
    r.rec_bytes = 0;
    if (from_records) { // the trajectory as the packed records a fused rollout wrote (whole records: the 1v1 kernels)
        susnet_record_layout_t lay;
        if (int rc = susnet_record_layout_of(env, io->record_format, &lay)) return rc;
        if (lay.record_bytes == 0 || lay.planar || lay.n_obs_segments != 1)
            return fail(env, SUSNET_E_INVALID, "susnet_ring_append: reads packed records where the handle stores them whole (the 1v1 kernels); the "
                                               "multi-agent kernels' planar records go through the separate trajectory tensors");
        r.rec_bytes = lay.record_bytes; r.rec_obs = lay.off_obs; r.rec_act = lay.off_actions; r.rec_rew = lay.off_rewards;
        r.rec_done = lay.off_done; r.rec_trunc = lay.off_truncated; r.rec_packed = lay.flags_packed;
    }
    const int64_t total = (int64_t)io->n_ticks * r.B;
    r.n0 = total > io->max_size ? total - io->max_size : 0; // (earlier rows would be overwritten by later ones of this same launch)
    r.n1 = total;
    r.n0_t = r.n0 / r.B;
    r.n0_b = (int32_t)(r.n0 % r.B);
    r.pos_n0 = (io->idx + r.n0) % io->max_size;
    if (r.n1 - r.n0 + r.B + 64 >= (1ll << 32)) return fail(SUSNET_E_INVALID, "susnet_ring_append: more than 2^32 rows in one launch");
    // the row images of k_ring_append: states, next_states (bytes), rewards (f32), actions (bytes), done, imposters (i16); a wave
    // takes 64 rows, or 32 / 16 / 8 when the window is long (trajectory_size x S bytes per row, twice): the reference's
    // ReplayBuffer accepts any trajectory_size (replay_memory.py:33-44)
    auto images = [&](size_t R) {
        return 2 * ((R * (size_t)io->trajectory_size * (size_t)r.S + 15) & ~(size_t)15) + R * r.A * 4 + ((R * r.A + 15) & ~(size_t)15) + 64 +
               R * r.n_imp * 2 + 16;
    };
    hipStream_t st = static_cast<hipStream_t>(stream);
    // a (ticks x envs) tile per wave where the window is short enough for the tile's lanes to fetch the Tw ticks ahead of it and the
    // images fit; else 64 (32 / 16 / 8) consecutive rows per wave
    r.rows_per_wave = 64;
    r.tile_log2e = 0;
    const int te = env->ring_tile;
    const size_t Tw = (size_t)io->trajectory_size;
    const size_t tile_lds = te ? ((((size_t)(64 / te) + Tw) * te * r.S + 15) & ~(size_t)15) + ((((size_t)(64 / te) + Tw) * te + 15) & ~(size_t)15) +
                                     2 * ((64 * Tw * r.S + 15) & ~(size_t)15) + 64 * (size_t)r.A * 4 + ((64 * (size_t)r.A + 15) & ~(size_t)15) + 64 +
                                     ((64 * (size_t)r.n_imp * 2 + 15) & ~(size_t)15) + (64 / te) * sizeof(RingRun)
                                : 0;
    if (te && Tw * te <= 64 && tile_lds <= 32 * 1024 && r.A >= 2) {
        r.tile_log2e = te == 8 ? 3 : te == 16 ? 4 : 5;
        const int64_t t_first = r.n0 / r.B, tiles_t = (io->n_ticks - t_first + 64 / te - 1) / (64 / te), tiles_b = (r.B + te - 1) / te;
        if (tiles_t * tiles_b > 0x7fffffffll) return fail(SUSNET_E_INVALID, "susnet_ring_append: too many tiles for one launch");
        if (from_records) hipLaunchKernelGGL(k_ring_append_tile<true>, dim3((unsigned)(tiles_t * tiles_b)), dim3(64), tile_lds, st, r);
        else hipLaunchKernelGGL(k_ring_append_tile<false>, dim3((unsigned)(tiles_t * tiles_b)), dim3(64), tile_lds, st, r);
    } else {
        while (r.rows_per_wave > 8 && images((size_t)r.rows_per_wave) > 64 * 1024) r.rows_per_wave /= 2;
        const size_t sh = images((size_t)r.rows_per_wave);
        if (sh > 64 * 1024) return fail(SUSNET_E_INVALID, "susnet_ring_append: trajectory_size x state size too large (8 rows of the window exceed 64 KiB)");
        const int64_t waves = (r.n1 - r.n0 + r.rows_per_wave - 1) / r.rows_per_wave;
        if (from_records) hipLaunchKernelGGL(k_ring_append<true>, dim3((unsigned)waves), dim3(64), sh, st, r);
        else hipLaunchKernelGGL(k_ring_append<false>, dim3((unsigned)waves), dim3(64), sh, st, r);
    }
    if (from_records) hipLaunchKernelGGL(k_ring_window<true>, dim3((unsigned)((r.B + 63) / 64)), dim3(64), 0, st, r);
    else hipLaunchKernelGGL(k_ring_window<false>, dim3((unsigned)((r.B + 63) / 64)), dim3(64), 0, st, r);
    HIP_TRY(hipGetLastError());
    return SUSNET_OK;
}

// susnet_state_window_push: the acting loop's raw window one tick on, in place -- k_ring_window<false> for ONE tick on a feed slot's
// pointers (it reads of RingArgs only io.window / obs / done / truncated / trajectory_size / n_ticks, B and S)
extern "C" int susnet_state_window_push(susnet_env *env, uint8_t *window, int32_t T, int32_t S, int64_t n, const uint8_t *obs, const uint8_t *done,
                                        const uint8_t *truncated, void *stream) {
    const std::string who = "susnet_state_window_push: ";
    if (!env) return fail(SUSNET_E_INVALID, who + "null env");
    if (T < 1 || T > 8) return fail(SUSNET_E_INVALID, who + "T = " + std::to_string(T) + ": windows of 1 .. 8 states are served");
    if (S != env->layout.obs_raw_size)
        return fail(SUSNET_E_INVALID, who + "S = " + std::to_string(S) + ": the handle's flattened state has " + std::to_string(env->layout.obs_raw_size) + " bytes (obs_raw_size)");
    if (n != env->c.B) return fail(SUSNET_E_INVALID, who + "n = " + std::to_string(n) + ": one window per environment of the handle (batch = " + std::to_string(env->c.B) + ")");
    if (!window) return fail(SUSNET_E_INVALID, who + "null window");
    if (!obs) return fail(SUSNET_E_INVALID, who + "null obs");
    if (!done) return fail(SUSNET_E_INVALID, who + "null done");
    if (!truncated) return fail(SUSNET_E_INVALID, who + "null truncated");
    RingArgs r = {};
    r.io.window = window;
    r.io.obs = obs;
    r.io.done = done;
    r.io.truncated = truncated;
    r.io.trajectory_size = T;
    r.io.n_ticks = 1;
    r.B = n;
    r.A = env->c.A;
    r.S = S;
    hipLaunchKernelGGL(k_ring_window<false>, dim3((unsigned)((r.B + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), r);
    HIP_TRY(hipGetLastError());
    return SUSNET_OK;
}
