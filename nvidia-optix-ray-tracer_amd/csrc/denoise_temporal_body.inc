// denoise_temporal_body.inc -- the statements of the temporal mode's reprojection and blend: the body of k_denoise_temporal (denoise.hip),
// of k_denoise_temporal_linked (denoise_link.hip) and of k_denoise_temporal_by_prim (denoise_link_prim.hip).  denoise_temporal_body.h has the definition and the names this expects in scope.
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.width * a.height) return;
    const float4 c = a.color[p];
    const uint32_t inst = a.inst[p];
    const float nan = __builtin_nanf("");
    float4 acc = c;
    float len = 0.0f;
    float2 mom = make_float2(0.0f, 0.0f);
    float2 mo = make_float2(nan, nan);
    uint2 id = make_uint2(kMissPrim, 0u);
    if (inst != kMissPrim) {
        const float4 h = a.tuvp[p];
        const uint32_t prim = __float_as_uint(h.w);
        id = make_uint2(inst, prim);
        len = 1.0f;
        float lc = 0.0f;
        if (kMoments) { lc = luminance(c); mom = make_float2(lc, lc * lc); }
        uint32_t pinst = inst;                                     // the instance's index in the history
        if constexpr (kLinked) pinst = prev_index[inst];
        const float *sv = nullptr;                                 // by primitive: the vertices of the instance's BLAS in the history
        if constexpr (kByPrim) sv = ((const float *const __attribute__((address_space(1))) *)prev_verts)[inst];
        if (a.has_history && (!kLinked || pinst != kNoInstance)) {
            const RayRec ray = a.rays[p];
            const float hp[3] = {ray.o.x + ray.d.x * h.x, ray.o.y + ray.d.y * h.x, ray.o.z + ray.d.z * h.x};      // hit_point
            float po[3], pw[3];
            xf_point(a.inst_inv + 12 * (size_t)inst, hp, po);
            if constexpr (kByPrim) {
                // the material point (prim, u, v) of the previous BLAS, hit_normal's vertex order (trav_common.h).  Every lane loads a
                // triangle -- the rigid ones (sv == NULL) nine floats of their own world -> object row, which are there -- and the
                // position is selected: lanes of one wave sit on both paths, and the projection below stands once
                const global_floats tv = sv ? (global_floats)sv + 9 * (size_t)prim : (global_floats)(a.inst_inv + 12 * (size_t)inst);
                const float va[3] = {tv[0], tv[1], tv[2]}, vb[3] = {tv[3], tv[4], tv[5]}, vc[3] = {tv[6], tv[7], tv[8]};
                const float bw = (1.0f - h.y) - h.z;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const float pb = (va[k] * bw + vb[k] * h.y) + vc[k] * h.z; po[k] = sv ? pb : po[k]; }
            }
            xf_point(a.prev_xf + 12 * (size_t)pinst, po, pw);
            const V3 r = mk3(pw[0] - a.prev_center[0], pw[1] - a.prev_center[1], pw[2] - a.prev_center[2]);
            const V3 U = mk3(a.prev_U[0], a.prev_U[1], a.prev_U[2]), V = mk3(a.prev_V[0], a.prev_V[1], a.prev_V[2]);
            const V3 W = mk3(a.prev_W[0], a.prev_W[1], a.prev_W[2]);
            const float s = dot3(r, W) / dot3(W, W);
            if (s > 0.0f) {
                const float fw = (float)a.width, fh = (float)a.height;
                const float aspect = fw / fh;
                const float ndcx = (dot3(r, U) / dot3(U, U)) / (s * aspect);
                const float ndcy = (dot3(r, V) / dot3(V, V)) / s;
                const float xp = ((ndcx + 1.0f) * 0.5f) * fw - 0.5f, yp = ((ndcy + 1.0f) * 0.5f) * fh - 0.5f;
                const float zp = sqrtf(dot3(r, r));
                mo = make_float2(xp, yp);
                const float x0 = floorf(xp), y0 = floorf(yp);
                const float fx = xp - x0, fy = yp - y0, gx = 1.0f - fx, gy = 1.0f - fy;
                const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
                size_t q[4]; bool in[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float qx = x0 + (float)(k & 1), qy = y0 + (float)(k >> 1);
                    in[k] = qx >= 0.0f && qx <= fw - 1.0f && qy >= 0.0f && qy <= fh - 1.0f;
                    const float cx = fminf(fmaxf(qx, 0.0f), fw - 1.0f), cy = fminf(fmaxf(qy, 0.0f), fh - 1.0f);      // (NaN -> 0)
                    q[k] = (size_t)(uint32_t)cy * a.width + (size_t)(uint32_t)cx;
                }
                uint2 qid[4]; float qz[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { qid[k] = a.prev_id[q[k]]; qz[k] = __uint_as_float(a.prev_guides[q[k]].w); }
                float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool take = in[k] && qid[k].x == pinst && qid[k].y == prim && fabsf(qz[k] - zp) <= a.depth_tolerance * zp;
                    if (take) {
                        const float4 ha = a.prev_accum[q[k]];
                        const float hl = a.prev_length[q[k]];
                        sw = sw + w[k];
                        sr = sr + w[k] * ha.x; sg = sg + w[k] * ha.y; sb = sb + w[k] * ha.z;
                        sl = sl + w[k] * hl;
                        if (kMoments) { const float2 hm = a.prev_moments[q[k]]; sm1 = sm1 + w[k] * hm.x; sm2 = sm2 + w[k] * hm.y; }
                    }
                }
                if (sw > 0.0f) {
                    const float hr = sr / sw, hg = sg / sw, hb = sb / sw;
                    len = fminf(sl / sw + 1.0f, a.max_history);
                    const float alpha = fmaxf(1.0f / len, a.alpha_min);
                    acc = make_float4(hr + alpha * (c.x - hr), hg + alpha * (c.y - hg), hb + alpha * (c.z - hb), c.w);
                    if (kMoments) { const float h1 = sm1 / sw, h2 = sm2 / sw; mom = make_float2(h1 + alpha * (mom.x - h1), h2 + alpha * (mom.y - h2)); }
                }
            }
        }
    }
    a.accum[p] = acc;
    a.length[p] = len;
    a.id[p] = id;
    a.motion[p] = mo;
    if (kMoments) a.moments[p] = mom;
