// the dense Q-network kernel (susnet_dense.h: susnet_mlp_forward) -- a translation unit of its own, default scheduling like the other
// Q-network units
#include "susnet_dense.h"

#include "susnet_host.h" // lds_opt_in

namespace susnet {

__global__ __launch_bounds__(kDnThreads) void k_qnet_dense(DenseArgs a) {
    extern __shared__ float dn_smem[];
    const int t = threadIdx.x, lane = t & 63, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nl = a.n_dims - 1;
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kDnRows;
        for (int l = 0; l < nl; l++) {
            const int dk = a.d[l], dn = a.d[l + 1];
            const float *W = a.W[l], *bias = a.B[l];
            const bool last = l == nl - 1;
            const float slope = last ? 1.0f : a.A[l][0];
            const float *zin = dn_smem + ((l & 1) ? 0 : a.buf1); // what layer l - 1 wrote
            float *zout = dn_smem + ((l & 1) ? a.buf1 : 0);
            const int items = ((dn + 31) >> 5) * 2;
            for (int it = wave; it < items; it += kDnWaves) {
                const int n0 = (it >> 1) * 32, st = it & 1;
                const int64_t s = base + st * 32 + i;
                const bool svalid = s < a.n;
                dn_f32x16 acc;
                if (l == 0) {
                    const float *xrow = a.rows + (size_t)(svalid ? s : a.n - 1) * dk;
                    acc = dn_block<true>(W, bias, dk, dn, n0, st, xrow, svalid, nullptr, lane);
                } else {
                    acc = dn_block<false>(W, bias, dk, dn, n0, st, nullptr, svalid, zin, lane);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int u = n0 + dn_row(r, lane);
                    if (u < dn) {
                        if (last) {
                            if (svalid) a.q[(size_t)s * dn + u] = acc[r];
                        } else {
                            zout[dn_lds(u, st * 32 + i)] = dn_prelu(acc[r], slope);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

size_t qnet_dense_lds(DenseArgs &a) {
    int w0 = 0, w1 = 0; // widest output of the layers that write buffer 0 (1st, 3rd, ..) / buffer 1; the last layer writes q_out
    for (int l = 0; l + 2 < a.n_dims; l++) {
        int &w = (l & 1) ? w1 : w0;
        w = a.d[l + 1] > w ? a.d[l + 1] : w;
    }
    a.buf1 = w0 * kDnRows;
    return (size_t)(w0 + w1) * kDnRows * sizeof(float);
}

hipError_t qnet_dense_launch(DenseArgs a, hipStream_t st) {
    const size_t lds = qnet_dense_lds(a);
    if (lds > kDnLdsNoOptIn) { // the opt-in to a large dynamic LDS block: once per device, off the per-tick path after that
        static LdsOptIn opted;
        if (hipError_t e = lds_opt_in(reinterpret_cast<const void *>(&k_qnet_dense), 2 * kDnMaxHidden * kDnRows * 4, opted)) return e;
    }
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    hipLaunchKernelGGL(k_qnet_dense, dim3((unsigned)(tiles < kDnMaxGrid ? tiles : kDnMaxGrid)), dim3(kDnThreads), lds, st, a);
    return hipGetLastError();
}

} // namespace susnet
