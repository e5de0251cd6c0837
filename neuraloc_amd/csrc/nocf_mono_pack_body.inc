// nocf_mono_pack_body.inc -- the body of mono_pack_kernel as a text fragment (see nocf_pack_body.inc): the one-CU kernels' images and plan
// record.  Included with `mp`, `P`, `ws` in scope and PACK_BID / PACK_NBLK defined, by mono_pack_kernel and mono_ens_pack_kernel.
    float4* ws4 = reinterpret_cast<float4*>(ws);
    const int m = mp.pp.m, D1 = mp.pp.D1, r = mp.pp.r, KBM = mp.KBM, KBD = mp.KBD;
    const long nW = (long)KBM * KBM * 64, nK1 = (long)KBM * KBD * 64, nK4 = (long)KBD * KBM * 64, nAZ = (long)KBD * 64, nAT = (long)KBD * 64;
    const long total = 2 * nW + nK1 + nK4 + nAZ + nAT;
    const long stride = (long)PACK_NBLK * blockDim.x;
    for (long idx = (long)PACK_BID * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        long q = idx, dst;
        const int lane = idx & 63;
        if (idx < 2 * nW) {
            const bool third = idx >= nW;
            q = (third ? idx - nW : idx) >> 6;
            const int kb = q % KBM, mt = q / KBM;
            const int o = 16 * mt + (lane & 15);
            for (int e = 0; e < 4; ++e) {
                const int k = 16 * kb + 4 * (lane >> 4) + e;
                if (o < m && k < m) v[e] = third ? P.K[(long)k * m + o] : P.K[(long)o * m + k];
            }
            dst = (third ? mp.oW3 : mp.oW2) + (third ? idx - nW : idx);
        } else if (idx < 2 * nW + nK1) {
            q = (idx - 2 * nW) >> 6;
            const int kb = q % KBD, mt = q / KBD;
            const int o = 16 * mt + (lane & 15);
            for (int e = 0; e < 4; ++e) {
                const int k = 16 * kb + 4 * (lane >> 4) + e;
                if (o < m && k < D1) v[e] = P.K0[(long)o * D1 + k];
            }
            dst = mp.oK1 + (idx - 2 * nW);
        } else if (idx < 2 * nW + nK1 + nK4) {
            q = (idx - 2 * nW - nK1) >> 6;
            const int kb = q % KBM, dt = q / KBM;
            const int dim = 16 * dt + (lane & 15);
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * kb + 4 * (lane >> 4) + e;
                if (i < m && dim < D1) v[e] = P.K0[(long)i * D1 + dim];
            }
            dst = mp.oK4 + (idx - 2 * nW - nK1);
        } else if (idx < 2 * nW + nK1 + nK4 + nAZ) {
            const int kb = (idx - 2 * nW - nK1 - nK4) >> 6;
            const int row = lane & 15;
            for (int e = 0; e < 4; ++e) {
                const int k = 16 * kb + 4 * (lane >> 4) + e;
                if (row < r && k < D1) v[e] = P.A[(long)row * D1 + k];
            }
            dst = mp.oAZ + (idx - 2 * nW - nK1 - nK4);
        } else {
            const int dt = (idx - 2 * nW - nK1 - nK4 - nAZ) >> 6;
            const int dim = 16 * dt + (lane & 15);
            for (int e = 0; e < 4; ++e) {
                const int row = 4 * (lane >> 4) + e;
                if (row < r && dim < D1) v[e] = P.A[(long)row * D1 + dim];
            }
            dst = mp.oAT + (idx - 2 * nW - nK1 - nK4 - nAZ);
        }
        ws4[dst] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (PACK_BID == 0 && threadIdx.x < sizeof(MonoPlan) / 4) {
        const unsigned* src = reinterpret_cast<const unsigned*>(&mp);
        unsigned v = src[threadIdx.x];
        if (P.cbp && threadIdx.x == (offsetof(MonoPlan, pp) + offsetof(DevPlan, cb)) / 4) v = __float_as_uint(*P.cbp);
        reinterpret_cast<unsigned*>(ws + mp.pp.oPlan)[threadIdx.x] = v;
    }
