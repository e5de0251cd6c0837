// nocf_pack_body.inc -- the body of pack_kernel as a text fragment: the statements that lay out the per-tile images, the padded vectors, the
// copy of A and the plan record in a workspace.  Included (with `pl`, `P`, `ws` in scope and PACK_BID / PACK_NBLK naming the block's index and
// count on the axis the work is spread over) by pack_kernel and by the one-CU ensemble's batched pack (mono_ens_pack_kernel, nocf_mono.inc),
// which runs it once per member.  A fragment and not a function: pack_kernel then compiles to what it always was.
    float4* ws4 = reinterpret_cast<float4*>(ws);
    const long nW0f = (long)pl.MB * pl.KQ1 * 64;       // opening:  B[k][j] = K0[j][k]
    const long nW0b = (long)pl.DB * pl.KQm * 64;       // closing:  B[k][i] = K0[k][i]
    const long nWl = (long)pl.MB * pl.KQm * 64;
    const long nLayers = pl.nTh - 1;
    const long total4 = nW0f + nW0b + 2 * nLayers * nWl;
    const long stride = (long)PACK_NBLK * blockDim.x;
    for (long idx = (long)PACK_BID * blockDim.x + threadIdx.x; idx < total4; idx += stride) {
        float v[4];
        long dst;
        if (idx < nW0f) {
            long q = idx;
            const int lane = q & 63; q >>= 6;
            const int kq = q % pl.KQ1, cb = q / pl.KQ1;
            const int j = cb * 64 + lane;
            for (int e = 0; e < 4; ++e) {
                const int k = kq * 4 + e;
                v[e] = (j < pl.m && k < pl.D1) ? P.K0[(long)j * pl.D1 + k] : 0.f;
            }
            dst = pl.oW0f + idx;
        } else if (idx < nW0f + nW0b) {
            long q = idx - nW0f;
            const int lane = q & 63; q >>= 6;
            const int kq = q % pl.KQm, cb = q / pl.KQm;
            const int i = cb * 64 + lane;
            for (int e = 0; e < 4; ++e) {
                const int k = kq * 4 + e;
                v[e] = (k < pl.m && i < pl.D1) ? P.K0[(long)k * pl.D1 + i] : 0.f;
            }
            dst = pl.oW0b + (idx - nW0f);
        } else {
            const long q = idx - nW0f - nW0b;
            const int layer = q / (2 * nWl);             // 0 -> reference layer 1
            long w = q - (long)layer * 2 * nWl;
            const int back = w >= nWl;
            if (back) w -= nWl;
            const int lane = w & 63; const long ww = w >> 6;
            const int kq = ww % pl.KQm, cb = ww / pl.KQm;
            const float* Kl = P.K + (long)layer * pl.m * pl.m;
            const int a = cb * 64 + lane;
            for (int e = 0; e < 4; ++e) {
                const int k = kq * 4 + e;
                float val = 0.f;
                if (a < pl.m && k < pl.m) val = back ? Kl[(long)k * pl.m + a]    // backward: B[j][col] = K[j][col]
                                                     : Kl[(long)a * pl.m + k];   // forward:  B[k][j]   = K[j][k]
                v[e] = val;
            }
            dst = (back ? pl.oWb : pl.oWf) + (long)layer * pl.strideW + w;
        }
        ws4[dst] = make_float4(v[0], v[1], v[2], v[3]);
    }
    // padded vectors
    const long nb0 = (long)pl.MB * 64, nb = nLayers * pl.MB * 64, nw = (long)pl.MB * 64, ncw = (long)pl.DB * 64;
    const long totalv = nb0 + nb + nw + ncw;
    for (long idx = (long)PACK_BID * blockDim.x + threadIdx.x; idx < totalv; idx += stride) {
        float val = 0.f;
        long dst;
        if (idx < nb0) { if (idx < pl.m) val = P.b0[idx]; dst = pl.ob0 + idx; }
        else if (idx < nb0 + nb) {
            const long q = idx - nb0; const int layer = q / (pl.MB * 64); const int c = q % (pl.MB * 64);
            if (c < pl.m) val = P.b[(long)layer * pl.m + c];
            dst = pl.ob + q;
        } else if (idx < nb0 + nb + nw) { const long q = idx - nb0 - nb; if (q < pl.m) val = P.w[q]; dst = pl.ow + q; }
        else { const long q = idx - nb0 - nb - nw; if (q < pl.D1) val = P.cw[q]; dst = pl.ocw + q; }
        ws[dst] = val;
    }
    for (long idx = (long)PACK_BID * blockDim.x + threadIdx.x; idx < (long)pl.r * pl.D1; idx += stride)
        ws[pl.oA + idx] = P.A[idx];
    // the plan itself, for the kernels that read it through a pointer
    if (PACK_BID == 0 && threadIdx.x < sizeof(DevPlan) / 4) {
        const unsigned* src = reinterpret_cast<const unsigned*>(&pl);
        unsigned v = src[threadIdx.x];
        if (P.cbp && threadIdx.x == offsetof(DevPlan, cb) / 4) v = __float_as_uint(*P.cbp);
        reinterpret_cast<unsigned*>(ws + pl.oPlan)[threadIdx.x] = v;
    }
