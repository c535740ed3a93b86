// susnet_mlp_train_grad_body.h -- the body of k_mlp_train_grad and k_mlp_train_sweep_grad (inst_mlp_train.hip includes it into both): ONE text,
// so workgroup (g, k) of a sweep does what workgroup g of learner k's own call does.  It names, as kernel arguments or as locals of the same
// names: MlpTrainBatch b, MlpTrainNet net, prm, tgt, lists, counts, agent, team, gamma, partial, zsave_all, step.  No include guard.
    extern __shared__ float lds[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int count = counts[2 * agent + team];
    if (count == 0) return; // an empty team takes no step (train.py:101): k_train_adam does nothing either
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    if (blockIdx.x == 0 && t == 0) step[0] += 1.0f; // (k_train_adam reads it after this launch)
    const int nl = net.nl, n_out = net.d[nl], F = net.d[0];
    float *out = partial + (size_t)blockIdx.x * net.Pp;
    float *zsave = zsave_all + (size_t)blockIdx.x * net.Z;
    float lacc = 0.0f, sacc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float inv_n = 2.0f / (float)count; // mse_loss backward: 2 (x - y) / numel
    int32_t *pos = reinterpret_cast<int32_t *>(lds + kMtOPos);
    int32_t *rid = reinterpret_cast<int32_t *>(lds + kMtORow);
    int32_t *act = reinterpret_cast<int32_t *>(lds + kMtOAct);
    const float *zq = lds + (((nl - 1) & 1) ? kMtOH1 : kMtOH0); // the last layer's output
    if ((int64_t)blockIdx.x * kTrTS >= count) // no tile: an all-zero partial (slopes and loss below)
        for (int p = t; p < net.P; p += kTrThreads) out[p] = 0.0f;
    for (int tile = blockIdx.x; (int64_t)tile * kTrTS < count; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int base = tile * kTrTS, nvalid = count - base < kTrTS ? count - base : kTrTS;
        if (t < kTrTS) {
            int64_t s = t < nvalid ? list[base + t] : 0;
            s = s < 0 ? 0 : (s >= b.n ? b.n - 1 : s);
            int64_t r = b.idx[s];
            r = r < 0 ? 0 : (r >= b.max_size ? b.max_size - 1 : r);
            pos[t] = (int32_t)s;
            rid[t] = (int32_t)r;
        }
        __syncthreads();
        // target network on the next states: y = r + gamma max_a Q'(s', a); y = r where done (train.py:121-134)
        mt_forward<false>(net, tgt, b.next_feat, pos, nvalid, lds, nullptr, t, wave, lane);
        if (t < kTrTS) {
            float y = 0.0f;
            int a = 0;
            if (t < nvalid) {
                const int64_t r = rid[t];
                float m = zq[t];
                for (int j = 1; j < n_out; j++) m = fmaxf(m, zq[j * kTrSP + t]);
                const float rew = b.rewards[r * b.A + agent];
                y = b.dones[r] ? rew : rew + gamma * m;
                a = (int)b.actions[r * b.A + agent];
                a = a < 0 ? 0 : (a >= n_out ? n_out - 1 : a);
            }
            lds[kMtOY + t] = y;
            act[t] = a;
        }
        __syncthreads();
        // online network on the states, hidden pre-activations kept in the slice
        mt_forward<true>(net, prm, b.feat, pos, nvalid, lds, zsave, t, wave, lane);
        { // dL/dQ (rows n_out) into the last layer's dZ buffer: 2 (Q - y) / n at the taken action, 0 elsewhere and on padding columns
            float *dq = lds + (((nl - 1) & 1) ? kMtODA : kMtODB);
            for (int e = t; e < n_out * kTrTS; e += kTrThreads) {
                const int j = e / kTrTS, s = e % kTrTS;
                float g = 0.0f;
                if (s < nvalid && j == act[s]) g = inv_n * (zq[j * kTrSP + s] - lds[kMtOY + s]);
                dq[j * kTrSP + s] = g;
            }
            if (t < nvalid) {
                const float diff = zq[act[t] * kTrSP + t] - lds[kMtOY + t];
                lacc += diff * diff;
            }
        }
        __syncthreads();
        // backward, last layer .. first: dz of layer l in DA (l odd) or DB (l even), dh into the other
#pragma unroll
        for (int l = kMtMaxLayers - 1; l >= 0; l--) {
            if (l < nl) {
                const float *dz = lds + ((l & 1) ? kMtODA : kMtODB);
                float *dh = lds + ((l & 1) ? kMtODB : kMtODA);
                float *zin = lds + ((l & 1) ? kMtOH0 : kMtOH1); // the pre-activations of layer l's input (l > 0)
                const int dk = net.d[l], dn = net.d[l + 1];
                float slope_in = 1.0f;
                if (l > 0) {
                    slope_in = prm[net.oA[l > 0 ? l - 1 : 0]];
                    const float *src = zsave + net.zo[l > 0 ? l - 1 : 0];
                    for (int e = t; e < dk * kTrTS; e += kTrThreads) zin[(e >> 5) * kTrSP + (e & 31)] = src[e];
                    __syncthreads();
                }
                // weight gradient of layer l, tile by tile: dW[n][k] += sum_s dz[n][s] h_in[k][s]
                const int KT = (dk + 31) / 32, tiles = ((dn + 31) / 32) * KT;
                for (int g = wave; g < tiles; g += kTrWaves) {
                    const int n0 = (g / KT) * 32, k0 = (g % KT) * 32;
                    const int k = k0 + (lane & 31), kc = k < dk ? k : dk - 1;
                    tr_f32x16 acc = {};
                    acc = tr_mfma([&](int i, int p) { return n0 + i < dn ? dz[(n0 + i) * kTrSP + p] : 0.0f; },
                                  [&](int p, int j) {
                                      if (l == 0) {
                                          const float x = b.feat[(size_t)pos[p] * F + kc];
                                          return (k < dk && p < nvalid) ? x : 0.0f;
                                      }
                                      const float z = zin[kc * kTrSP + p];
                                      return k < dk ? tr_prelu(z, slope_in) : 0.0f;
                                  },
                                  kTrTS, acc, lane);
                    float *wg = out + net.oW[l];
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int n = n0 + tr_row(r, lane);
                        if (n < dn && k < dk) {
                            float *w = wg + (size_t)n * dk + k;
                            *w = first ? acc[r] : *w + acc[r];
                        }
                    }
                }
                if (t < dn) { // bias gradient
                    float s = 0.0f;
                    for (int j = 0; j < kTrTS; j++) s += dz[t * kTrSP + j];
                    float *w = out + net.oB[l] + t;
                    *w = first ? s : *w + s;
                }
                if (l > 0) {
                    tr_backward_layer(prm + net.oW[l], dk, dn, dz, dh, wave, lane);
                    __syncthreads();
                    // through the PReLU of layer l's input: dz = z > 0 ? dh : a dh; d slope = sum over z <= 0 of z dh (torch's prelu backward)
                    for (int e = t; e < dk * kTrTS; e += kTrThreads) {
                        const int k = e / kTrTS, s = e % kTrTS;
                        const float z = zin[k * kTrSP + s], g = dh[k * kTrSP + s];
                        const bool pz = z > 0.0f;
                        dh[k * kTrSP + s] = pz ? g : slope_in * g;
                        sacc[l > 0 ? l - 1 : 0] += pz ? 0.0f : z * g;
                    }
                }
                __syncthreads();
            }
        }
    }
    // slopes and loss: fixed-shape tree sums over the workgroup
    float *red = lds;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMtMaxLayers; q++) {
        if (q < nl) { // q < nl - 1: the slope behind layer q; q == nl - 1: the loss
            tr_block_sum(q < nl - 1 ? sacc[q < 6 ? q : 5] : lacc, red, t);
            if (t == 0) out[q < nl - 1 ? net.oA[q < 6 ? q : 5] : net.P] = red[0];
            __syncthreads();
        }
    }
