// The body of k_spatial_rnn / k_spatial_rnn_dropout (susnet_spatial.h): included by inst_qnet_spatial.hip inside each KERNEL with
// SP_RNN_DROPOUT defined 0 / 1: no include guard.  Text, not a template, as susnet_spatial_train_rnn_body.h is: the plain kernel's machine
// code is then what the text without the #if branches compiles to.  The including kernel provides `a` (SpatialRnnArgs) and, with
// SP_RNN_DROPOUT, `dr` (SpActDrop).
// SP_RNN_DROPOUT: nn.RNN's training-mode forward.  Behind the L + 1 rotating buffers lie one (L = 2) or two buffers D that hold m[l][t] *
// h_l[t], written beside h_l[t] at the tanh write -- registers 4 q .. 4 q + 3 of the accumulator are four consecutive units of one row, one
// Philox block (sp_drop4_at) -- and read by layer l + 1 in place of `below`; layer l's own recurrence reads the undropped h_l[t] from the
// rotation and the head the undropped top layer.  Layer l writes D[l & 1] and reads D[(l - 1) & 1]: a step's waves read and write D between
// the same two barriers, so one buffer would be a race from L = 3 on.
    extern __shared__ float sr_smem[];
    const int t_ = threadIdx.x, lane = t_ & 63, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t_ >> 6);
    const int L = a.L, H = a.H, nb = L + 1, nl = a.n_dims - 1;
    const int64_t tiles = (a.n + kDnRows - 1) / kDnRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kDnRows;
#if SP_RNN_DROPOUT
        // the mask's coordinates of this lane's two rows (tile halves st = 0 / 1): env = row / agents, agent = row % agents
        int64_t d_env[2];
        int d_agent[2];
#pragma unroll
        for (int st = 0; st < 2; st++) {
            const int64_t s = base + st * 32 + i, sc = s < a.n ? s : a.n - 1;
            d_env[st] = sc / dr.agents;
            d_agent[st] = (int)(sc - d_env[st] * dr.agents);
        }
#endif
        int c = 0; // step t L + l writes buffer c mod (L + 1); h_{l-1}[t] is one buffer back, h_l[t-1] one buffer on
        for (int t = 0; t < a.T; t++) {
            for (int l = 0; l < L; l++, c = c + 1 == nb ? 0 : c + 1) {
                float *hout = sr_smem + (size_t)c * a.buf;
#if SP_RNN_DROPOUT
                const float *below = sr_smem + (size_t)(nb + ((l + 1) & 1)) * a.buf; // m[l-1][t] h_{l-1}[t]  (not read at l = 0)
                float *dout = sr_smem + (size_t)(nb + (l & 1)) * a.buf;
#else
                const float *below = sr_smem + (size_t)(c == 0 ? nb - 1 : c - 1) * a.buf;
#endif
                const float *before = sr_smem + (size_t)(c + 1 == nb ? 0 : c + 1) * a.buf;
                const float *Wih = a.w_ih[l], *Whh = a.w_hh[l], *bih = a.b_ih[l], *bhh = a.b_hh[l];
                const int items = ((H + 31) >> 5) * 2;
                for (int it = wave; it < items; it += kDnWaves) {
                    const int n0 = (it >> 1) * 32, st = it & 1;
                    const int64_t s = base + st * 32 + i;
                    const bool svalid = s < a.n;
                    dn_f32x16 acc = dn_bias(bih, bhh, H, n0, lane);
                    if (l == 0) {
                        const float *xrow = a.rnn_in + ((size_t)(svalid ? s : a.n - 1) * a.T + t) * a.R;
                        acc = dn_chain<true>(acc, Wih, a.R, H, n0, st, xrow, svalid, nullptr, lane);
                    } else {
                        acc = dn_chain<false>(acc, Wih, H, H, n0, st, nullptr, svalid, below, lane);
                    }
                    if (t > 0) acc = dn_chain<false>(acc, Whh, H, H, n0, st, nullptr, svalid, before, lane);
#if SP_RNN_DROPOUT
                    if (l < L - 1) { // (wave-uniform) the top layer's output is not dropped
                        const uint64_t g = (uint64_t)(dr.row_base + (st ? d_env[1] : d_env[0]));
                        const int agent = st ? d_agent[1] : d_agent[0];
#pragma unroll
                        for (int q = 0; q < 4; q++) { // registers 4 q .. 4 q + 3: four consecutive units, one Philox block
                            const int u4 = n0 + dn_row(4 * q, lane);
                            if (u4 < H) {
                                float m[4];
                                sp_drop4_at(dr.k0, dr.k1, dr.off_lo, dr.off_hi, dr.thr, dr.scale, dr.net, agent, g, t, l, u4 >> 2, m);
#pragma unroll
                                for (int j = 0; j < 4; j++) {
                                    const int u = u4 + j;
                                    if (u < H) {
                                        const float hv = sp_tanh(acc[4 * q + j]);
                                        hout[dn_lds(u, st * 32 + i)] = hv;
                                        dout[dn_lds(u, st * 32 + i)] = m[j] * hv;
                                    }
                                }
                            }
                        }
                    } else
#endif
                    {
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int u = n0 + dn_row(r, lane);
                            if (u < H) hout[dn_lds(u, st * 32 + i)] = sp_tanh(acc[r]);
                        }
                    }
                }
                __syncthreads();
            }
        }
        // the head (dqn.py:298-299) on h_{L-1}[T-1], which the last step left one buffer back; its layers alternate between that buffer and c
        int zi = c == 0 ? nb - 1 : c - 1, zo = c;
        for (int l = 0; l < nl; l++) {
            const int dk = a.d[l], dn = a.d[l + 1];
            const float *W = a.W[l], *bias = a.B[l];
            const bool last = l == nl - 1;
            const float slope = last ? 1.0f : a.A[l][0];
            const float *zin = sr_smem + (size_t)zi * a.buf;
            float *zout = sr_smem + (size_t)zo * a.buf;
            const int items = ((dn + 31) >> 5) * 2;
            for (int it = wave; it < items; it += kDnWaves) {
                const int n0 = (it >> 1) * 32, st = it & 1;
                const int64_t s = base + st * 32 + i;
                const bool svalid = s < a.n;
                const dn_f32x16 acc = dn_block<false>(W, bias, dk, dn, n0, st, nullptr, svalid, zin, lane);
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
            const int sw = zi;
            zi = zo;
            zo = sw;
        }
    }
