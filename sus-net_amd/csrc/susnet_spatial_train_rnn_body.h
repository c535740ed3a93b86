// susnet_spatial_train_rnn_body.h -- the body of k_sp_train_rnn and of k_sp_train_rnn_dropout (inst_spatial_train.hip), included ONCE PER
// KERNEL with SP_TRAIN_DROPOUT defined 0 / 1: no include guard.  Text, not a template: a kernel body that reads the argument structs through
// a function's reference parameters is compiled to other machine code than one that names the kernel arguments (the loads lose what the
// compiler knows of the kernel-argument segment), and k_sp_train_rnn must stay the code it was.  In scope: the kernel's arguments and,
// with SP_TRAIN_DROPOUT, `dr` (SpDrop) and `ms`.
// SP_TRAIN_DROPOUT: both recurrences under their masks (net 1 the target's, net 0 the online one's), whose multipliers m[l][t] live in the
// workgroup's slice msl ([l][t][unit][32], l < L - 1; the target's first, then overwritten by the online network's, which the backward pass
// reads): dz[l][t] = (1 - h^2) (m[l][t] (W_ih[l+1]^T dz[l+1][t]) + ..), dW_ih[l+1] += dz[l+1][t] (m[l][t] h[l][t])^T.
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int count = counts[2 * agent + team];
    if (count == 0) return; // an empty team takes no step (train.py:101): k_train_adam does nothing either
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    if (blockIdx.x == 0 && tid == 0) step[0] += 1.0f; // (k_train_adam reads it after this launch)
    const SpTrainNet &net = *netp;
    const MlpTrainNet &hd = net.head;
    const int nl = hd.nl, n_out = hd.d[nl], H = net.H, L = net.L, T = net.T, R = net.R, Rc = net.Rc;
    float *out = partial + (size_t)blockIdx.x * net.Pp;
    const size_t slice = (size_t)L * T * H * kTrTS;
    float *hs = ws.hs + (size_t)blockIdx.x * slice, *ds = ws.ds + (size_t)blockIdx.x * slice;
    float *zsave = ws.zs + (size_t)blockIdx.x * hd.Z;
#if SP_TRAIN_DROPOUT
    float *msl = ms + (size_t)blockIdx.x * ((size_t)(L - 1) * T * H * kTrTS);
#endif
    float lacc = 0.0f;
    float *red = lds + kStORed;
    const float inv_n = 2.0f / (float)count; // mse_loss backward: 2 (x - y) / numel
    int32_t *rid = reinterpret_cast<int32_t *>(lds + kStORow);
    int32_t *act = reinterpret_cast<int32_t *>(lds + kStOAct);
    const float *zq = lds + (((nl - 1) & 1) ? kStOH1 : kStOH0); // the last layer's output
    if ((int64_t)blockIdx.x * kTrTS >= count) // no tile: an all-zero partial behind the convolutions' part (slopes and loss below)
        for (int p = net.oWih[0] + tid; p < net.P; p += kTrThreads) out[p] = 0.0f;
    for (int tile = blockIdx.x; (int64_t)tile * kTrTS < count; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int base = tile * kTrTS, nvalid = count - base < kTrTS ? count - base : kTrTS;
        const int64_t j0 = base;
        if (tid < kTrTS) {
            const int64_t s = st_clamp(tid < nvalid ? list[base + tid] : 0, b.n);
            rid[tid] = (int32_t)st_clamp(b.idx[s], b.max_size);
        }
        __syncthreads();
        // target network on the next states: y = r + gamma max_a Q'(s', a); y = r where done (train.py:121-134)
#if SP_TRAIN_DROPOUT
        st_forward<false, true>(net, tgt, ws.Xt, j0, nvalid, hs, lds, nullptr, tid, wave, lane, &dr, 1, list, b.n, msl);
#else
        st_forward<false, false>(net, tgt, ws.Xt, j0, nvalid, hs, lds, nullptr, tid, wave, lane, nullptr, 0, nullptr, 0, nullptr);
#endif
        if (tid < kTrTS) {
            float y = 0.0f;
            int a = 0;
            if (tid < nvalid) {
                const int64_t r = rid[tid];
                float m = zq[tid];
                for (int j = 1; j < n_out; j++) m = fmaxf(m, zq[j * kTrSP + tid]);
                const float rew = b.rewards[r * b.A + agent];
                y = b.dones[r] ? rew : rew + gamma * m;
                a = (int)b.actions[r * b.A + agent];
                a = a < 0 ? 0 : (a >= n_out ? n_out - 1 : a);
            }
            lds[kStOY + tid] = y;
            act[tid] = a;
        }
        __syncthreads();
        // online network on the states: every h[l][t] in hs, the head's hidden pre-activations in zsave
#if SP_TRAIN_DROPOUT
        st_forward<true, true>(net, prm, ws.X, j0, nvalid, hs, lds, zsave, tid, wave, lane, &dr, 0, list, b.n, msl);
#else
        st_forward<true, false>(net, prm, ws.X, j0, nvalid, hs, lds, zsave, tid, wave, lane, nullptr, 0, nullptr, 0, nullptr);
#endif
        { // dL/dQ into the last layer's dZ buffer: 2 (Q - y) / n at the taken action, 0 elsewhere and on padding columns
            float *dq = lds + (((nl - 1) & 1) ? kStODA : kStODB);
            for (int e = tid; e < n_out * kTrTS; e += kTrThreads) {
                const int j = e / kTrTS, s = e % kTrTS;
                float g = 0.0f;
                if (s < nvalid && j == act[s]) g = inv_n * (zq[j * kTrSP + s] - lds[kStOY + s]);
                dq[j * kTrSP + s] = g;
            }
            if (tid < nvalid) {
                const float diff = zq[act[tid] * kTrSP + tid] - lds[kStOY + tid];
                lacc += diff * diff;
            }
        }
        __syncthreads();
        // the head's backward, last layer .. first, as k_mlp_train_grad: dz of layer l in DA (l odd) or DB (l even), dh into the other;
        // layer 0's input is the top hidden state (no activation in front of it), and its dh -- left in DA -- is the recurrence's
        for (int l = nl - 1; l >= 0; l--) {
            {
                const float *dz = lds + ((l & 1) ? kStODA : kStODB);
                float *dh = lds + ((l & 1) ? kStODB : kStODA);
                float *zin = lds + ((l & 1) ? kStOH0 : kStOH1);
                const int dk = hd.d[l], dn = hd.d[l + 1];
                const float slope_in = l > 0 ? prm[hd.oA[l - 1]] : 1.0f;
                {
                    const float *src = l > 0 ? zsave + hd.zo[l - 1] : hs + ((size_t)((L - 1) * T + T - 1) * H) * kTrTS;
                    for (int e = tid; e < dk * kTrTS; e += kTrThreads) zin[(e >> 5) * kTrSP + (e & 31)] = src[e];
                    __syncthreads();
                }
                const int KT = (dk + 31) / 32, tiles = ((dn + 31) / 32) * KT;
                for (int g = wave; g < tiles; g += kTrWaves) {
                    const int n0 = (g / KT) * 32, k0 = (g % KT) * 32;
                    const int k = k0 + (lane & 31), kc = k < dk ? k : dk - 1;
                    tr_f32x16 acc = {};
                    acc = tr_mfma([&](int i, int p) { return n0 + i < dn ? dz[(n0 + i) * kTrSP + p] : 0.0f; },
                                  [&](int p, int j) {
                                      const float z = zin[kc * kTrSP + p];
                                      return k < dk ? (l == 0 ? z : tr_prelu(z, slope_in)) : 0.0f;
                                  },
                                  kTrTS, acc, lane);
                    float *wg = out + hd.oW[l];
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int n = n0 + tr_row(r, lane);
                        if (n < dn && k < dk) {
                            float *w = wg + (size_t)n * dk + k;
                            *w = first ? acc[r] : *w + acc[r];
                        }
                    }
                }
                if (tid < dn) { // bias gradient
                    float s = 0.0f;
                    for (int j = 0; j < kTrTS; j++) s += dz[tid * kTrSP + j];
                    float *w = out + hd.oB[l] + tid;
                    *w = first ? s : *w + s;
                }
                tr_backward_layer(prm + hd.oW[l], dk, dn, dz, dh, wave, lane);
                __syncthreads();
                if (l > 0) { // through the PReLU of layer l's input (torch's prelu backward); the slope's gradient: a fixed-shape tree sum per tile
                    float sl = 0.0f;
                    for (int e = tid; e < dk * kTrTS; e += kTrThreads) {
                        const int k = e / kTrTS, s = e % kTrTS;
                        const float z = zin[k * kTrSP + s], g = dh[k * kTrSP + s];
                        const bool pz = z > 0.0f;
                        dh[k * kTrSP + s] = pz ? g : slope_in * g;
                        sl += pz ? 0.0f : z * g;
                    }
                    tr_block_sum(sl, red, tid);
                    if (tid == 0) {
                        float *w = out + hd.oA[l - 1];
                        *w = first ? red[0] : *w + red[0];
                    }
                    __syncthreads();
                }
            }
        }
        const float *dhead = lds + kStODA; // [H][kTrSP]
        // back through time: dz[l][t] = (1 - h^2) (W_ih[l+1]^T dz[l+1][t] + W_hh[l]^T dz[l][t+1] (+ dhead at the top, last step))
        const int kt_count = (H + 31) / 32;
        for (int t = T - 1; t >= 0; t--) {
            for (int l = L - 1; l >= 0; l--) {
                const float *Wup = prm + net.oWih[l < L - 1 ? l + 1 : l], *Whh = prm + net.oWhh[l];
                const float *dzup = ds + ((size_t)((l < L - 1 ? l + 1 : l) * T + t) * H) * kTrTS;
                const float *dzfut = ds + ((size_t)(l * T + (t < T - 1 ? t + 1 : t)) * H) * kTrTS;
                const float *h = hs + ((size_t)(l * T + t) * H) * kTrTS;
                float *dzo = ds + ((size_t)(l * T + t) * H) * kTrTS;
                const bool top = l == L - 1 && t == T - 1;
                for (int kt = wave; kt < kt_count; kt += kTrWaves) {
                    const int k0 = kt * 32;
                    tr_f32x16 acc = {};
                    if (l < L - 1)
                        acc = tr_mfma([&](int i, int p) { return k0 + i < H ? Wup[(size_t)p * H + k0 + i] : 0.0f; },
                                      [&](int p, int j) { return dzup[p * kTrTS + j]; }, H, acc, lane);
#if SP_TRAIN_DROPOUT
                    if (l < L - 1) { // the gradient that came down through layer l + 1's input passes m[l][t]
                        const float *m = msl + ((size_t)(l * T + t) * H) * kTrTS;
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int k = k0 + tr_row(r, lane);
                            acc[r] *= m[(k < H ? k : H - 1) * kTrTS + (lane & 31)];
                        }
                    }
#endif
                    if (t < T - 1)
                        acc = tr_mfma([&](int i, int p) { return k0 + i < H ? Whh[(size_t)p * H + k0 + i] : 0.0f; },
                                      [&](int p, int j) { return dzfut[p * kTrTS + j]; }, H, acc, lane);
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int k = k0 + tr_row(r, lane), s = lane & 31;
                        if (k < H) {
                            const float g = acc[r] + (top ? dhead[k * kTrSP + s] : 0.0f);
                            const float hv = h[k * kTrTS + s];
                            dzo[k * kTrTS + s] = (1.0f - hv * hv) * g;
                        }
                    }
                }
                __syncthreads();
            }
        }
        { // gradient of the RNN input's convolution columns: dX[s][t][k] = sum_n W_ih[0][n][k] dz[0][t][n][s], k < Rc
            const float *W0 = prm + net.oWih[0];
            const int KT = (Rc + 31) / 32;
            for (int g = wave; g < T * KT; g += kTrWaves) {
                const int t = g / KT, k0 = (g % KT) * 32;
                const float *dz0 = ds + ((size_t)t * H) * kTrTS;
                tr_f32x16 acc = {};
                acc = tr_mfma([&](int i, int p) { return k0 + i < Rc ? W0[(size_t)p * R + k0 + i] : 0.0f; }, [&](int p, int j) { return dz0[p * kTrTS + j]; },
                              H, acc, lane);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int k = k0 + tr_row(r, lane), s = lane & 31;
                    if (k < Rc && s < nvalid) ws.dX[((size_t)(j0 + s) * T + t) * Rc + k] = acc[r];
                }
            }
        }
        // the recurrence's weight gradients, one product over all steps and the tile's rows per 32 x 32 block: p = 32 t + s
        for (int l = 0; l < L; l++) {
            const int dk = l == 0 ? R : H;
            const float *dzl = ds + ((size_t)(l * T) * H) * kTrTS;
            const float *hbelow = hs + ((size_t)((l > 0 ? l - 1 : 0) * T) * H) * kTrTS;
            const float *hown = hs + ((size_t)(l * T) * H) * kTrTS;
#if SP_TRAIN_DROPOUT
            const float *mbelow = msl + ((size_t)((l > 0 ? l - 1 : 0) * T) * H) * kTrTS;
#endif
            const int KT = (dk + 31) / 32, HT = (H + 31) / 32;
            for (int g = wave; g < HT * KT; g += kTrWaves) { // dW_ih[n][k] = sum_{t, s} dz[l][t][n][s] in[l][t][k][s]
                const int n0 = (g / KT) * 32, k0 = (g % KT) * 32;
                const int k = k0 + (lane & 31), kc = k < dk ? k : dk - 1;
                tr_f32x16 acc = {};
                acc = tr_mfma([&](int i, int p) { return n0 + i < H ? dzl[((size_t)(p >> 5) * H + n0 + i) * kTrTS + (p & 31)] : 0.0f; },
                              [&](int p, int j) {
                                  const int t = p >> 5, s = p & 31;
                                  float x;
                                  if (l == 0) x = s < nvalid ? ws.X[((size_t)(j0 + (s < nvalid ? s : 0)) * T + t) * R + kc] : 0.0f;
                                  else x = hbelow[((size_t)t * H + kc) * kTrTS + s];
#if SP_TRAIN_DROPOUT
                                  if (l > 0) x *= mbelow[((size_t)t * H + kc) * kTrTS + s];
#endif
                                  return k < dk ? x : 0.0f;
                              },
                              T * kTrTS, acc, lane);
                float *wg = out + net.oWih[l];
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = n0 + tr_row(r, lane);
                    if (n < H && k < dk) {
                        float *w = wg + (size_t)n * dk + k;
                        *w = first ? acc[r] : *w + acc[r];
                    }
                }
            }
            for (int g = wave; g < HT * HT; g += kTrWaves) { // dW_hh[n][k] = sum_{t >= 1, s} dz[l][t][n][s] h[l][t-1][k][s]
                const int n0 = (g / HT) * 32, k0 = (g % HT) * 32;
                const int k = k0 + (lane & 31), kc = k < H ? k : H - 1;
                tr_f32x16 acc = {};
                acc = tr_mfma([&](int i, int p) { return n0 + i < H ? dzl[((size_t)((p >> 5) + 1) * H + n0 + i) * kTrTS + (p & 31)] : 0.0f; },
                              [&](int p, int j) {
                                  const float x = hown[((size_t)(p >> 5) * H + kc) * kTrTS + (p & 31)];
                                  return k < H ? x : 0.0f;
                              },
                              (T - 1) * kTrTS, acc, lane);
                float *wg = out + net.oWhh[l];
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int n = n0 + tr_row(r, lane);
                    if (n < H && k < H) {
                        float *w = wg + (size_t)n * H + k;
                        *w = first ? acc[r] : *w + acc[r];
                    }
                }
            }
            if (tid < H) { // bias_ih and bias_hh: the same gradient
                float s = 0.0f;
                for (int p = 0; p < T * kTrTS; p++) s += dzl[((size_t)(p >> 5) * H + tid) * kTrTS + (p & 31)];
                float *w1 = out + net.oBih[l] + tid, *w2 = out + net.oBhh[l] + tid;
                const float v = first ? s : *w1 + s;
                *w1 = v;
                *w2 = v;
            }
        }
        __syncthreads(); // (the next tile rewrites rid, the slices and the LDS buffers)
    }
    // the loss: a fixed-shape tree sum over the workgroup
    __syncthreads();
    tr_block_sum(lacc, red, tid);
    if (tid == 0) out[net.P] = red[0];
