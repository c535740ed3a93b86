// the feature-window kernel (susnet_window.h: susnet_window_push) -- a translation unit of its own
#include "susnet_window.h"

namespace susnet {

__global__ __launch_bounds__(kWinThreads) void k_window_push(WindowArgs a) {
    const uint32_t F = (uint32_t)a.F, W = (uint32_t)a.T * F, keep = W - F; // dwords per segment / per row / taken over from src
    const int64_t chunks = (a.n + kWinChunkRows - 1) / kWinChunkRows;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t row0 = c * kWinChunkRows;
        const uint32_t rows = (uint32_t)(a.n - row0 < kWinChunkRows ? a.n - row0 : kWinChunkRows);
        const uint32_t count = rows * W; // <= 64 * 1024 dwords
        const uint32_t *__restrict__ src = a.src + row0 * W;
        const uint32_t *__restrict__ fresh = a.fresh + row0 * F;
        uint32_t *__restrict__ dst = a.dst + row0 * W;
        for (uint32_t i = threadIdx.x; i < count; i += kWinThreads) {
            const uint32_t r = i / W, j = i - r * W, k = j % F;
            bool ended = false;
            if (a.done) ended = a.done[row0 + r] != 0;
            if (a.truncated) ended = ended || a.truncated[row0 + r] != 0;
            dst[i] = (ended || j >= keep) ? fresh[r * F + k] : src[i + F];
        }
    }
}

hipError_t window_push_launch(const WindowArgs &a, hipStream_t st) {
    const int64_t chunks = (a.n + kWinChunkRows - 1) / kWinChunkRows;
    hipLaunchKernelGGL(k_window_push, dim3((unsigned)(chunks < kWinMaxGrid ? chunks : kWinMaxGrid)), dim3(kWinThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace susnet
