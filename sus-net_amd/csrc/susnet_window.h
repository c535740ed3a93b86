// susnet_window.h -- susnet_window_push: the trainer's state window (src/train.py:318-322, 388-389, 441-445) kept as FEATURE rows on the
// device.  A window is a row of T segments of F floats, oldest state first -- what MLP.forward flattens its [B, T, F] input into
// (src/models/dqn.py:86-90) and what susnet_mlp_forward / susnet_mlp_train_step read as a row of width T * F.  Per tick and row:
//
//   ended      dst = fresh x T                  (train.py:441-445: the window is refilled with the fresh first state)
//   otherwise  dst = src[F:] ++ fresh           (train.py:388-389: np.roll(-1), then the last slot is the new state)
//
//   k_window_push  OUT OF PLACE (the caller ping-pongs two buffers: no ordering between a wave's loads and stores of overlapping addresses
//                  is relied on).  A workgroup walks chunks of kWinChunkRows rows (grid-stride); a chunk of the window is one contiguous
//                  run of dwords, thread i of the workgroup takes dwords i, i + 256, ..: consecutive lanes store consecutive dwords.  Rows
//                  are only 4-byte aligned (F is arbitrary), so every access is one dword; values move as 32-bit patterns (NaN payloads and
//                  -0.0 survive).  Dword j of a row comes from fresh[j % F] if the row ended or j is in the last segment, else from
//                  src[j + F]: j + F < T F there, so nothing is read or written past a row.  No LDS, no atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/susnet.h"

namespace susnet {

constexpr int kWinThreads = 256, kWinChunkRows = 64, kWinMaxGrid = 4096, kWinMaxT = 8;

struct WindowArgs { // by value: the kernel's arguments
    const uint32_t *fresh; // [n][F]
    const uint8_t *done, *truncated; // [n] or nullptr
    const uint32_t *src;   // [n][T F]
    uint32_t *dst;         // [n][T F]
    int32_t T, F;
    int64_t n;
};

// the launch (inst_window.hip); `a` validated by the caller
hipError_t window_push_launch(const WindowArgs &a, hipStream_t st);

} // namespace susnet
