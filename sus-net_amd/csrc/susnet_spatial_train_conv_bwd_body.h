// susnet_spatial_train_conv_bwd_body.h -- the body of k_sp_train_conv_bwd and of k_sp_train_sweep_conv_bwd (inst_spatial_train.hip),
// included ONCE PER KERNEL: no include guard.  Text, not a template, for susnet_spatial_train_rnn_body.h's reason: k_sp_train_conv_bwd must
// stay the code it was.  In scope: b (SpTrainBatch), netp, ws (SpTrainWs), prm, lists, counts, agent, team, partial -- the kernel's
// arguments, or in the sweep form what the learner's table entry gives for them.
    const int tid = threadIdx.x;
    const int count = counts[2 * agent + team];
    if (count == 0) return;
    const SpTrainNet &net = *netp;
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    const int64_t nimg = (int64_t)count * net.T;
    float *out = partial + (size_t)blockIdx.x * net.Pp;
    const int k = net.k, last = net.n_conv - 1;
    // through the ReLUs and the transposed convolutions, top down; the gated gradient of every layer's output stays in the workspace
    for (int64_t img = blockIdx.x; img < nimg; img += gridDim.x) {
        for (int l = last; l >= 0; l--) {
            const float *y = l == last ? ws.X + (size_t)img * net.R : ws.act + (size_t)img * net.asz + net.aoff[l];
            float *d = l == last ? ws.dX + (size_t)img * net.Rc : ws.dact + (size_t)img * net.asz + net.aoff[l];
            for (int e = tid; e < net.sz[l + 1]; e += kStConvThreads) d[e] = y[e] > 0.0f ? d[e] : 0.0f; // relu'(0) = 0, as torch
            __syncthreads();
            if (l > 0) {
                float *din = ws.dact + (size_t)img * net.asz + net.aoff[l > 0 ? l - 1 : 0];
                const int si = net.size[l], so = net.size[l + 1], ci_n = net.ch[l], co_n = net.ch[l + 1], str = net.stride[l], pad = net.pad[l],
                          dil = net.dil[l];
                const float *W = prm + net.oCW[l];
                for (int e = tid; e < net.sz[l]; e += kStConvThreads) {
                    const int ci = e / (si * si), iy = (e / si) % si, ix = e % si;
                    float acc = 0.0f;
                    for (int co = 0; co < co_n; co++)
                        for (int ky = 0; ky < k; ky++) {
                            const int ny = iy + pad - ky * dil;
                            if (ny < 0 || ny % str != 0 || ny / str >= so) continue;
                            for (int kx = 0; kx < k; kx++) {
                                const int nx = ix + pad - kx * dil;
                                if (nx < 0 || nx % str != 0 || nx / str >= so) continue;
                                acc = fmaf(W[((co * ci_n + ci) * k + ky) * k + kx], d[(co * so + ny / str) * so + nx / str], acc);
                            }
                        }
                    din[e] = acc;
                }
                __syncthreads();
            }
        }
    }
    // weight and bias gradients: a thread per parameter, images then pixels in ascending order, stored once
    for (int l = 0; l <= last; l++) {
        const int si = net.size[l], so = net.size[l + 1], ci_n = net.ch[l], co_n = net.ch[l + 1], str = net.stride[l], pad = net.pad[l], dil = net.dil[l];
        const int nW = co_n * ci_n * k * k;
        for (int w = tid; w < nW + co_n; w += kStConvThreads) {
            const bool bias = w >= nW;
            const int co = bias ? w - nW : w / (ci_n * k * k), ci = bias ? 0 : (w / (k * k)) % ci_n, ky = bias ? 0 : (w / k) % k, kx = bias ? 0 : w % k;
            float acc = 0.0f;
            for (int64_t img = blockIdx.x; img < nimg; img += gridDim.x) {
                const float *d = (l == last ? ws.dX + (size_t)img * net.Rc : ws.dact + (size_t)img * net.asz + net.aoff[l]) + (size_t)co * so * so;
                if (bias) {
                    for (int e = 0; e < so * so; e++) acc += d[e];
                    continue;
                }
                const float *in;
                if (l == 0) {
                    const int64_t s = st_clamp(list[img / net.T], b.n);
                    in = b.spatial + s * b.sp_stride[0] + agent * b.sp_stride[1] + (img % net.T) * b.sp_stride[2];
                } else {
                    in = ws.act + (size_t)img * net.asz + net.aoff[l > 0 ? l - 1 : 0];
                }
                in += (size_t)ci * si * si;
                for (int oy = 0; oy < so; oy++) {
                    const int iy = oy * str - pad + ky * dil;
                    if (iy < 0 || iy >= si) continue;
                    for (int ox = 0; ox < so; ox++) {
                        const int ix = ox * str - pad + kx * dil;
                        if (ix < 0 || ix >= si) continue;
                        acc = fmaf(d[oy * so + ox], in[iy * si + ix], acc);
                    }
                }
            }
            out[bias ? net.oCB[l] + co : net.oCW[l] + w] = acc;
        }
    }
