// susnet_spatial_train_conv_body.h -- the body of k_sp_train_conv and of k_sp_train_sweep_conv (inst_spatial_train.hip), included ONCE PER
// KERNEL: no include guard.  Text, not a template, for susnet_spatial_train_rnn_body.h's reason: k_sp_train_conv must stay the code it was.
// In scope: b (SpTrainBatch), netp, ws (SpTrainWs), prm, tgt, lists, counts, agent, team -- the kernel's arguments, or in the sweep form
// what the learner's table entry gives for them.
    const int tid = threadIdx.x;
    const int count = counts[2 * agent + team];
    if (count == 0) return;
    const SpTrainNet &net = *netp;
    const int32_t *list = lists + ((int64_t)agent * 2 + team) * b.n;
    const int64_t nimg = (int64_t)count * net.T;
    float *slice = ws.tact + (size_t)blockIdx.x * 2 * net.maxsz;
    for (int64_t job = blockIdx.x; job < 2 * nimg; job += gridDim.x) {
        const bool target = job >= nimg;
        const int64_t img = target ? job - nimg : job;
        const int64_t j = img / net.T;
        const int step = (int)(img % net.T);
        const int64_t s = st_clamp(list[j], b.n);
        const float *P = target ? tgt : prm;
        const float *in = (target ? b.next_spatial : b.spatial) + s * b.sp_stride[0] + agent * b.sp_stride[1] + step * b.sp_stride[2];
        float *xrow = (target ? ws.Xt : ws.X) + (size_t)img * net.R;
        for (int l = 0; l < net.n_conv; l++) {
            float *out = l == net.n_conv - 1 ? xrow : (target ? slice + (l & 1) * net.maxsz : ws.act + (size_t)img * net.asz + net.aoff[l]);
            const int si = net.size[l], so = net.size[l + 1], ci_n = net.ch[l], k = net.k, str = net.stride[l], pad = net.pad[l], dil = net.dil[l];
            const float *W = P + net.oCW[l], *B = P + net.oCB[l];
            for (int e = tid; e < net.sz[l + 1]; e += kStConvThreads) {
                const int co = e / (so * so), oy = (e / so) % so, ox = e % so;
                float acc = B[co];
                for (int ci = 0; ci < ci_n; ci++)
                    for (int ky = 0; ky < k; ky++) {
                        const int iy = oy * str - pad + ky * dil;
                        if (iy < 0 || iy >= si) continue;
                        for (int kx = 0; kx < k; kx++) {
                            const int ix = ox * str - pad + kx * dil;
                            if (ix < 0 || ix >= si) continue;
                            acc = fmaf(W[((co * ci_n + ci) * k + ky) * k + kx], in[(ci * si + iy) * si + ix], acc);
                        }
                    }
                out[e] = acc > 0.0f ? acc : 0.0f;
            }
            __syncthreads();
            in = out;
        }
        if (net.Fn > 0) {
            const float *ns = (target ? b.next_non_spatial : b.non_spatial) + s * b.ns_stride[0] + agent * b.ns_stride[1] + step * b.ns_stride[2];
            for (int f = tid; f < net.Fn; f += kStConvThreads) xrow[net.Rc + f] = ns[f];
        }
    }
