// susnet_episodes.h -- per-episode returns and lengths from a [T][B] feed block (susnet_episode_stats): the trainer's episode bookkeeping.
//
// Reference behaviour (paths relative to the reference repo root):
//   G = reward + gamma * G             src/train.py:385-386   per agent, float64, the product rounded before the add
//   imposter / crew return, length     src/train.py:419-438   G[imposter_mask].mean(), G[~imposter_mask].mean() (numpy's summation order),
//                                                             t_episode + 1 steps; then G = 0, t_episode = 0
//
// B environments run in lockstep and restart inside the rollout launch, so the bookkeeping reads the feed block the rollout left on the
// device.  Per call three launches on one stream, whatever T and B are, no atomics, no host synchronisation:
//   k_episode_count   lane = environment, loop over the block's ticks: the number of episodes that end at (tick, wave of 64 envs), by ballot
//   k_episode_scan    ONE workgroup: exclusive scan of those counts in (tick, wave) order on top of the log's count -> the log position of
//                     each (tick, wave)'s first record; advances count / dropped
//   k_episode_write   lane = environment, G in registers, loop over the ticks: the update above; where the episode ends the lane's record
//                     goes to position[tick][wave] + (ended lanes below it in the wave) -- tick-major, env-minor, the order a host loop
//                     over ticks and envs appends in -- when that is inside the log; the carried G / t_episode go back to memory.  With
//                     an info log the feed's susnet_episode_info of that (tick, env) is copied to the same position of the parallel log
#pragma once

#include "susnet_device.h"

namespace susnet {

constexpr int kEpThreads = 256;      // k_episode_count / k_episode_write: 4 waves of 64 environments
constexpr int kEpScanThreads = 1024; // k_episode_scan: the one workgroup

struct EpisodeArgs {
    const float *rewards;     // [T][B][A]
    const uint8_t *done;      // [T][B]
    const uint8_t *truncated; // [T][B]
    const uint16_t *roles;    // [T][B] imposter bitmask of the episode that acted
    double *G;                // carry [A][B]
    int32_t *t_episode;       // carry [B]
    susnet_episode_record *log;
    int64_t capacity;
    int64_t *count, *dropped;
    int32_t *counts;          // workspace [T][W]
    int64_t *position;        // workspace [T][W]
    double gamma;
    int64_t tick_base;
    int32_t T, B, W;
    const susnet_episode_info *info; // [T][B] the feed's info records (valid where done | truncated), or NULL
    susnet_episode_info *info_log;   // [capacity] parallel to log, or NULL
};

__global__ __launch_bounds__(kEpThreads) void k_episode_count(EpisodeArgs p) {
    const int b = blockIdx.x * kEpThreads + threadIdx.x, w = b >> 6;
    const bool valid = b < p.B;
    for (int t = 0; t < p.T; t++) {
        const size_t i = (size_t)t * p.B + b;
        const bool ended = valid && (p.done[i] | p.truncated[i]);
        const unsigned long long m = __ballot(ended);
        if ((threadIdx.x & 63) == 0 && w < p.W) p.counts[(size_t)t * p.W + w] = __popcll(m); // (the last workgroup may hold waves past B)
    }
}

// exclusive scan of counts[0 .. n) (n = T * W, tick-major) on top of *count; thread i takes the i-th contiguous chunk
__global__ __launch_bounds__(kEpScanThreads) void k_episode_scan(EpisodeArgs p) {
    extern __shared__ long long ep_part[]; // [kEpScanThreads / 64]
    const long long n = (long long)p.T * p.W, chunk = (n + kEpScanThreads - 1) / kEpScanThreads;
    const long long i0 = (long long)threadIdx.x * chunk < n ? (long long)threadIdx.x * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
    const long long base = *p.count, dropped = *p.dropped;
    long long mine = 0;
    for (long long i = i0; i < i1; i++) mine += p.counts[i];
    // inclusive scan over the threads: within the wave by shuffles, across the 16 waves through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const long long v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) ep_part[wave] = incl;
    __syncthreads(); // (also: every thread has read *count / *dropped before thread 0 rewrites them)
    long long before = 0, total = 0;
    for (int k = 0; k < kEpScanThreads / 64; k++) {
        if (k < wave) before += ep_part[k];
        total += ep_part[k];
    }
    long long run = base + before + incl - mine;
    for (long long i = i0; i < i1; i++) {
        p.position[i] = run;
        run += p.counts[i];
    }
    if (threadIdx.x == 0) {
        const long long want = base + total, kept = want < p.capacity ? want : p.capacity;
        *p.count = kept;
        *p.dropped = dropped + (want - kept);
    }
}

// float64 add / multiply / divide that stay what they are: hipcc contracts a * b + c into a fused multiply-add by default (and HIP's
// __dmul_rn / __dadd_rn are plain operators, contracted like any other), numpy rounds the product first
__device__ __forceinline__ double ep_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double ep_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double ep_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// numpy's float64 add.reduce over n <= 12 contiguous values (pairwise_sum: below 8 values one by one from 0.0; else eight accumulators
// combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest added one by one), divided by n: ndarray.mean().  n == 0: NaN, as numpy.
template <int A>
__device__ __forceinline__ double ep_mean(const double (&v)[A], int n) {
    double s = 0.0;
    if constexpr (A >= 8) {
        if (n >= 8) {
            s = ep_add(ep_add(ep_add(v[0], v[1]), ep_add(v[2], v[3])), ep_add(ep_add(v[4], v[5]), ep_add(v[6], v[7])));
#pragma unroll
            for (int j = 8; j < A; j++)
                if (j < n) s = ep_add(s, v[j]);
            return ep_div(s, (double)n);
        }
    }
#pragma unroll
    for (int j = 0; j < A; j++)
        if (j < n) s = ep_add(s, v[j]);
    return ep_div(s, (double)n);
}

// the values of the agents whose bit in `mask` is set, in agent order, as a dense prefix (G[mask] of numpy); every index is a
// compile-time constant after unrolling: registers, no private memory
template <int A>
__device__ __forceinline__ double ep_team_mean(const double (&G)[A], unsigned mask) {
    double v[A];
#pragma unroll
    for (int j = 0; j < A; j++) v[j] = 0.0;
    int k = 0;
#pragma unroll
    for (int a = 0; a < A; a++) {
        const bool in = (mask >> a) & 1u;
#pragma unroll
        for (int j = 0; j <= a; j++)
            if (in && k == j) v[j] = G[a];
        k += in ? 1 : 0;
    }
    return ep_mean<A>(v, k);
}

template <int A>
__global__ __launch_bounds__(kEpThreads) void k_episode_write(EpisodeArgs p) {
    const int b = blockIdx.x * kEpThreads + threadIdx.x, w = b >> 6, lane = threadIdx.x & 63;
    const bool valid = b < p.B;
    double G[A];
    int32_t te = 0;
#pragma unroll
    for (int a = 0; a < A; a++) G[a] = valid ? p.G[(size_t)a * p.B + b] : 0.0;
    if (valid) te = p.t_episode[b];
    for (int t = 0; t < p.T; t++) {
        const size_t i = (size_t)t * p.B + b;
        uint8_t dn = 0, tr = 0;
        if (valid) {
            dn = p.done[i];
            tr = p.truncated[i];
            const float *r = p.rewards + i * A;
#pragma unroll
            for (int a = 0; a < A; a++) G[a] = ep_add((double)r[a], ep_mul(p.gamma, G[a])); // train.py:386: product rounded, then the sum
        }
        const bool ended = valid && (dn | tr);
        const unsigned long long m = __ballot(ended);
        if (ended) {
            const long long pos = p.position[(size_t)t * p.W + w] + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < p.capacity) {
                const unsigned all = (1u << A) - 1u, imp = (unsigned)p.roles[i] & all;
                susnet_episode_record rec;
                rec.imposter_return = ep_team_mean<A>(G, imp);
                rec.crew_return = ep_team_mean<A>(G, ~imp & all);
                rec.tick = p.tick_base + t;
                rec.env = b;
                rec.length = te + 1;
                rec.ended_by = (dn ? SUSNET_EPISODE_DONE : 0) | (tr ? SUSNET_EPISODE_TRUNCATED : 0);
                rec.reserved = 0;
                p.log[pos] = rec;
                if (p.info_log != nullptr) { // the episode's info counters, to the same position: one 16-byte load and store
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    reinterpret_cast<u32x4 *>(p.info_log)[pos] = reinterpret_cast<const u32x4 *>(p.info)[i];
                }
            }
#pragma unroll
            for (int a = 0; a < A; a++) G[a] = 0.0;
            te = 0;
        } else {
            te += 1;
        }
    }
    if (valid) {
#pragma unroll
        for (int a = 0; a < A; a++) p.G[(size_t)a * p.B + b] = G[a];
        p.t_episode[b] = te;
    }
}

} // namespace susnet
