// tools/store_patterns.hip -- what the write path of an MI355X does with the store patterns of the fused rollouts.
//
// 1 024 single-wave workgroups (one per SIMD, the geometry of bench.py's headline launch: 65 536 envs x 512 ticks), every lane
// one "environment"; per tick a lane burns VALU instructions (the step's arithmetic stand-in) and stores R bytes of "record".
// Patterns (R = 20 unless stated):
//   aos20      st128 + st32 at lane * 20 within the tick's slab (the round-2 packed record of cfg2)
//   aos32      2 x st128 at lane * 32 (record padded to a 32-byte sector)
//   aos16      st128 at lane * 16 (a 16-byte record: every store instruction covers 1 024 contiguous bytes)
//   soa16_4    st128 at chunk0 + lane * 16, st32 at chunk1 + lane * 4 (wave-blocked: [tick][wave][16 B x 64 | 4 B x 64])
//   lds20      the 20-byte records of the wave transposed through LDS, written as 80 contiguous 16-byte pieces (64 + 16 lanes)
//   aos40/80   cfg3 / cfg4 sized records as 16-byte stores at lane * R (+ an 8-byte tail)
//   none       no stores (the arithmetic alone)
//   ring16     the aos16 bytes through an LDS ring: 256 workgroups of 4 arithmetic waves + 1 writer wave (320 threads, one group per CU).
//              An arithmetic wave writes its tick's 1 KiB to LDS (ds_write_b128) instead of memory; every P ticks (the ring period) all five
//              waves meet at ONE s_barrier and the arithmetic waves flip to the other buffer; the writer wave reads the buffer just filled and
//              stores it (4 x st128 per tick, 4 KiB contiguous) while the next period fills the other one.  Barrier-only: no flags, no polling.
// Store cache policy (aos16 and ring16 only): aux 0 = default, 2 = nt (non-temporal), 16 = sc1 (write-through).
// build: hipcc -O3 --offload-arch=gfx950 -o store_patterns tools/store_patterns.hip
// run:   ./store_patterns [valu_per_tick ...]          every pattern, default policy
//        ./store_patterns ring [valu_per_tick ...]     none / aos16 / ring16 at periods 4, 6, 12, each store policy, 3 repetitions (min .. max)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(void *p, uint32_t bytes) { return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)bytes, 0x00020000); }

enum { P_NONE, P_AOS20, P_AOS32, P_AOS16, P_SOA16_4, P_LDS20, P_AOS40, P_AOS80, P_SOA40, P_SOA80, P_COUNT };
static const char *kNames[] = {"none", "aos20", "aos32", "aos16", "soa16_4", "lds20", "aos40", "aos80", "soa40", "soa80"};
static const int kBytes[] = {0, 20, 32, 16, 20, 20, 40, 80, 40, 80};

template <int P, int AUX = 0>
__global__ __launch_bounds__(64) void k_store(uint8_t *out, uint32_t slab, int ticks, int valu, uint32_t *sink) {
    __shared__ uint32_t lds[64 * 5 + 16];
    const uint32_t lane = threadIdx.x, wave = blockIdx.x;
    constexpr uint32_t R = P == P_NONE ? 0 : (P == P_AOS20 || P == P_SOA16_4 || P == P_LDS20) ? 20 : P == P_AOS32 ? 32 : P == P_AOS16 ? 16 : (P == P_AOS40 || P == P_SOA40) ? 40 : 80;
    const __amdgpu_buffer_rsrc_t r = rsrc(out, slab * (uint32_t)ticks);
    uint32_t x = lane * 2654435761u + wave, y = wave ^ 0x9e3779b9u;
    const uint32_t wbase = wave * 64u * R;
    for (int t = 0; t < ticks; t++) {
        for (int k = 0; k < valu; k++) { x = x * 5u + y; y ^= x >> 7; } // (2 VALU per k, dependent)
        const uint32_t so = (uint32_t)t * slab;
        const u32x4 v = {x, y, x ^ y, x + y};
        if (P == P_AOS20) {
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 20u + so, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(x, r, wbase + lane * 20u + 16u, so, 0);
        } else if (P == P_AOS32) {
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 32u + so, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 32u + 16u + so, 0, 0);
        } else if (P == P_AOS16) {
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 16u + so, 0, AUX);
        } else if (P == P_SOA16_4) {
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 16u + so, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(x, r, wbase + 1024u + lane * 4u, so, 0);
        } else if (P == P_LDS20) {
            // records into LDS as they lie in memory (lane * 20 bytes), read back as 16-byte pieces
            uint32_t *mine = lds + lane * 5;
            mine[0] = v.x; mine[1] = v.y; mine[2] = v.z; mine[3] = v.w; mine[4] = x;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const u32x4 a = *reinterpret_cast<const u32x4 *>(lds + lane * 4);
            __builtin_amdgcn_raw_buffer_store_b128(a, r, wbase + lane * 16u + so, 0, 0);
            if (lane < 16) {
                const u32x4 b = *reinterpret_cast<const u32x4 *>(lds + 256 + lane * 4);
                __builtin_amdgcn_raw_buffer_store_b128(b, r, wbase + 1024u + lane * 16u + so, 0, 0);
            }
            __builtin_amdgcn_wave_barrier();
        } else if (P == P_AOS40) {
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 40u + so, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 40u + 16u + so, 0, 0);
            const u32x2 w = {x, y};
            __builtin_amdgcn_raw_buffer_store_b64(w, r, wbase + lane * 40u + 32u, so, 0);
        } else if (P == P_SOA40) {
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 16u + so, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + 1024u + lane * 16u + so, 0, 0);
            const u32x2 w = {x, y};
            __builtin_amdgcn_raw_buffer_store_b64(w, r, wbase + 2048u + lane * 8u, so, 0);
        } else if (P == P_AOS80) {
#pragma unroll
            for (int k = 0; k < 5; k++) __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + lane * 80u + 16u * k + so, 0, 0);
        } else if (P == P_SOA80) {
#pragma unroll
            for (int k = 0; k < 5; k++) __builtin_amdgcn_raw_buffer_store_b128(v, r, wbase + 1024u * k + lane * 16u + so, 0, 0);
        }
    }
    if (x == 0x12345u && y == 0x54321u) sink[0] = x; // keep the arithmetic
}

// ring16 (see the header).  LDS, dynamic: 2 buffers x period ticks x 4 waves x 1 KiB.  The period schedule is a function of (ticks, period)
// alone and both roles walk it, so all five waves execute the same barriers.
constexpr uint32_t kRingTickBytes = 4u * 1024u;
template <int AUX>
__global__ __launch_bounds__(320) void k_ring(uint8_t *out, uint32_t slab, int ticks, int valu, int period, uint32_t *sink) {
    extern __shared__ u32x4 ring[]; // [2][period][4 waves][64 lanes] x 16 bytes
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, group = blockIdx.x, wave = 4u * group + w;
    const uint32_t buf_words = (uint32_t)period * (kRingTickBytes / 16u);
    uint32_t x = lane * 2654435761u + wave, y = wave ^ 0x9e3779b9u;
    if (w < 4u) {
        uint32_t buf = 0;
        for (int t0 = 0; t0 < ticks; t0 += period) {
            const int len = ticks - t0 < period ? ticks - t0 : period;
            u32x4 *dst = ring + buf * buf_words + w * 64u + lane;
            for (int sl = 0; sl < len; sl++) {
                for (int k = 0; k < valu; k++) { x = x * 5u + y; y ^= x >> 7; }
                const u32x4 v = {x, y, x ^ y, x + y};
                dst[(uint32_t)sl * 256u] = v;
            }
            __syncthreads(); // (the LDS writes waited for, then s_barrier)
            buf ^= 1u;
        }
        if (x == 0x12345u && y == 0x54321u) sink[0] = x;
    } else {
        const __amdgpu_buffer_rsrc_t r = rsrc(out, slab * (uint32_t)ticks);
        const uint32_t gbase = group * kRingTickBytes + lane * 16u;
        uint32_t buf = 0;
        for (int t0 = 0; t0 < ticks; t0 += period) {
            const int len = ticks - t0 < period ? ticks - t0 : period;
            __syncthreads(); // buffer `buf` is full; the reads of the other one were waited for before its stores were issued
            const u32x4 *src = ring + buf * buf_words + lane;
#pragma unroll 2
            for (int sl = 0; sl < len; sl++) {
                u32x4 v[4];
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = src[(uint32_t)sl * 256u + q * 64u];
#pragma unroll
                for (int q = 0; q < 4; q++) __builtin_amdgcn_raw_buffer_store_b128(v[q], r, gbase + q * 1024u + (uint32_t)(t0 + sl) * slab, 0, AUX); // (offset field 0: BufDst::st128)
            }
            buf ^= 1u;
        }
    }
}

static float time_launches(const std::function<void()> &launch, int reps) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 2; i++) launch();
    hipEventRecord(e0);
    for (int i = 0; i < reps; i++) launch();
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return hipGetLastError() == hipSuccess ? ms / reps : -1.f;
}

template <int AUX>
static float run_ring(uint8_t *out, size_t cap, int waves, int ticks, int valu, int period, uint32_t *sink, int reps) {
    const uint32_t slab = (uint32_t)waves * 64u * 16u;
    const size_t lds = 2u * (size_t)period * kRingTickBytes;
    if ((size_t)slab * ticks > cap || waves % 4 != 0 || lds > 160u * 1024u) { printf("ring16: bad geometry\n"); return -1.f; }
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ring<AUX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1.f;
    return time_launches([&] { hipLaunchKernelGGL(k_ring<AUX>, dim3(waves / 4), dim3(320), lds, 0, out, slab, ticks, valu, period, sink); }, reps);
}

template <int AUX>
static float run_aos16(uint8_t *out, int waves, int ticks, int valu, uint32_t *sink, int reps) {
    const uint32_t slab = (uint32_t)waves * 64u * 16u;
    return time_launches([&] { hipLaunchKernelGGL((k_store<P_AOS16, AUX>), dim3(waves), dim3(64), 0, 0, out, slab, ticks, valu, sink); }, reps);
}

// ring16 stores what aos16 stores, byte for byte (same x, y per wave and tick): compared once on the host
static bool ring_matches(uint8_t *out, int waves, int ticks, uint32_t *sink) {
    const size_t n = (size_t)waves * 64 * 16 * ticks;
    const uint32_t slab = (uint32_t)waves * 64u * 16u;
    std::vector<uint8_t> a(n), b(n);
    hipMemset(out, 0, n);
    hipLaunchKernelGGL((k_store<P_AOS16, 0>), dim3(waves), dim3(64), 0, 0, out, slab, ticks, 3, sink);
    hipMemcpy(a.data(), out, n, hipMemcpyDeviceToHost);
    for (int period : {4, 6, 12}) {
        hipMemset(out, 0, n);
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ring<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * period * (int)kRingTickBytes);
        hipLaunchKernelGGL(k_ring<0>, dim3(waves / 4), dim3(320), 2u * period * kRingTickBytes, 0, out, slab, ticks, 3, period, sink);
        if (hipMemcpy(b.data(), out, n, hipMemcpyDeviceToHost) != hipSuccess || a != b) return false;
    }
    return true;
}

static int main_ring(std::vector<int> valus, uint8_t *out, size_t cap, uint32_t *sink) {
    const int waves = 1024, ticks = 512, reps = 10, trials = 3;
    if (valus.empty()) valus = {0, 40, 60, 70, 80, 90, 100, 110, 120, 130, 140};
    if (!ring_matches(out, waves, 40, sink)) { printf("ring16 does not store the aos16 bytes\n"); return 1; }
    printf("{\"waves\": %d, \"ticks\": %d, \"reps_per_trial\": %d, \"trials\": %d, \"ring16_bytes_equal_aos16\": true, \"rows\": [\n", waves, ticks, reps, trials);
    bool first = true;
    auto row = [&](int valu, const char *name, int period, int aux, const std::function<float()> &f) {
        float lo = 1e30f, hi = 0.f, sum = 0.f;
        for (int i = 0; i < trials; i++) { const float ms = f(); lo = ms < lo ? ms : lo; hi = ms > hi ? ms : hi; sum += ms; }
        printf("%s {\"valu_per_tick\": %d, \"pattern\": \"%s\", \"period\": %d, \"aux\": %d, \"us_min\": %.1f, \"us_mean\": %.1f, \"us_max\": %.1f, \"cycles_per_tick_at_2.4GHz\": %.0f}",
               first ? " " : ",\n ", 2 * valu, name, period, aux, lo * 1e3, sum / trials * 1e3, hi * 1e3, sum / trials * 1e-3 / ticks * 2.4e9);
        first = false;
        fflush(stdout);
    };
    for (int valu : valus) {
        row(valu, "none", 0, 0, [&] { return time_launches([&] { hipLaunchKernelGGL((k_store<P_NONE>), dim3(waves), dim3(64), 0, 0, out, 4u, ticks, valu, sink); }, reps); });
        row(valu, "aos16", 0, 0, [&] { return run_aos16<0>(out, waves, ticks, valu, sink, reps); });
        row(valu, "aos16", 0, 2, [&] { return run_aos16<2>(out, waves, ticks, valu, sink, reps); });
        row(valu, "aos16", 0, 16, [&] { return run_aos16<16>(out, waves, ticks, valu, sink, reps); });
        for (int period : {4, 6, 12}) {
            row(valu, "ring16", period, 0, [&] { return run_ring<0>(out, cap, waves, ticks, valu, period, sink, reps); });
            row(valu, "ring16", period, 2, [&] { return run_ring<2>(out, cap, waves, ticks, valu, period, sink, reps); });
            row(valu, "ring16", period, 16, [&] { return run_ring<16>(out, cap, waves, ticks, valu, period, sink, reps); });
        }
    }
    printf("\n]}\n");
    return 0;
}

template <int P>
static float run(uint8_t *out, size_t cap, int waves, int ticks, int valu, uint32_t *sink, int reps) {
    const uint32_t slab = (uint32_t)waves * 64u * (uint32_t)kBytes[P];
    if ((size_t)slab * ticks > cap) { printf("%s: buffer too small\n", kNames[P]); return -1.f; }
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 2; i++) hipLaunchKernelGGL(k_store<P>, dim3(waves), dim3(64), 0, 0, out, slab ? slab : 4u, ticks, valu, sink);
    hipEventRecord(e0);
    for (int i = 0; i < reps; i++) hipLaunchKernelGGL(k_store<P>, dim3(waves), dim3(64), 0, 0, out, slab ? slab : 4u, ticks, valu, sink);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    return ms / reps;
}

int main(int argc, char **argv) {
    const int waves = 1024, ticks = 512, reps = 10;
    std::vector<int> valus;
    const bool ring = argc > 1 && std::string(argv[1]) == "ring";
    for (int i = ring ? 2 : 1; i < argc; i++) valus.push_back(atoi(argv[i]));
    const size_t cap = (size_t)waves * 64 * 80 * ticks;
    uint8_t *out; uint32_t *sink;
    if (hipMalloc(&out, cap) != hipSuccess || hipMalloc(&sink, 64) != hipSuccess) { printf("alloc failed\n"); return 1; }
    hipMemset(out, 0, cap);
    if (ring) return main_ring(valus, out, cap, sink);
    if (valus.empty()) valus = {0, 40, 120, 200};
    printf("{\"waves\": %d, \"ticks\": %d, \"rows\": [\n", waves, ticks);
    bool first = true;
    for (int valu : valus) {
        float ms[P_COUNT];
        ms[P_NONE] = run<P_NONE>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_AOS20] = run<P_AOS20>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_AOS32] = run<P_AOS32>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_AOS16] = run<P_AOS16>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_SOA16_4] = run<P_SOA16_4>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_LDS20] = run<P_LDS20>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_AOS40] = run<P_AOS40>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_AOS80] = run<P_AOS80>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_SOA40] = run<P_SOA40>(out, cap, waves, ticks, valu, sink, reps);
        ms[P_SOA80] = run<P_SOA80>(out, cap, waves, ticks, valu, sink, reps);
        for (int p = 0; p < P_COUNT; p++) {
            const double bytes = (double)waves * 64 * kBytes[p] * ticks;
            printf("%s {\"valu_per_tick\": %d, \"pattern\": \"%s\", \"record_bytes\": %d, \"us\": %.1f, \"GBs\": %.0f, \"cycles_per_tick_at_2.4GHz\": %.0f}",
                   first ? " " : ",\n ", 2 * valu, kNames[p], kBytes[p], ms[p] * 1e3, ms[p] > 0 ? bytes / (ms[p] * 1e-3) / 1e9 : 0.0, ms[p] * 1e-3 / ticks * 2.4e9);
            first = false;
        }
    }
    printf("\n]}\n");
    return 0;
}
