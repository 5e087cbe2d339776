// The trunk's body (trace_body.h): statements, included inside a kernel -- no include guard, no namespace.  The part behind f2 (the gi
// rows) is for the includers that name TRUNK_GI_ROW.

    // LayerNorm(F) statistics: mean, then the centred second moment
    float sum = 0.f;
    for (int T = 0; T < KT; ++T) {
        const f32x4 x = TRUNK_FEAT(TRUNK_KTILE(T));
        sum += (x[0] + x[1]) + (x[2] + x[3]);
    }
    const float mu = group_sum(sum) / (float)F;
    float sq = 0.f;
    for (int T = 0; T < KT; ++T) {
        const KTile kt = TRUNK_KTILE(T);
        const f32x4 x = TRUNK_FEAT(kt);
        for (int q = 0; q < 4; ++q)
            if (q < kt.nv) { const float d = x[q] - mu; sq = fmaf(d, d, sq); }
    }
    const float rstd = 1.0f / sqrtf(group_sum(sq) / (float)F + 1e-5f);

    // fc1 over the row's K tiles; operands from the fragment-major pack (iplan_ac_pack_fc1) or from the arena in place
    const float* __restrict__ pkw = which ? a.packed_critic : a.packed_actor;
    if (pkw) pkw += (int64_t)net * a.packed_s_net;
    const float* __restrict__ pkg = pkw ? pkw + (int64_t)KT * 1024 : nullptr;
    const float* __restrict__ pkb = pkw ? pkg + (int64_t)KT * 16 : nullptr;
    const float* fnw = P + nw.off[IPLAN_AC_FN_W];
    const float* fnb = P + nw.off[IPLAN_AC_FN_B];
    const float* W1 = P + nw.off[IPLAN_AC_FC1_W];
    auto kload = [&](int T, TrunkOps& o) {
        o.kt = TRUNK_KTILE(T);
        o.x = TRUNK_FEAT(o.kt);
        if (pkw) {
            o.gm = *reinterpret_cast<const f32x4*>(pkg + T * 16 + 4 * g);
            o.bt = *reinterpret_cast<const f32x4*>(pkb + T * 16 + 4 * g);
            for (int oo = 0; oo < PT; ++oo) o.wf[oo] = *reinterpret_cast<const f32x4*>(pkw + ((int64_t)(T * PT + oo) * 64 + l) * 4);
            return;
        }
        o.gm = kcols(o.kt, fnw);
        o.bt = kcols(o.kt, fnb);
        for (int oo = 0; oo < PT; ++oo) o.wf[oo] = kcols(o.kt, W1 + (int64_t)(16 * oo + n) * F);
    };
    f32x4 acc[PT], part[PT];
    for (int o = 0; o < PT; ++o) { acc[o] = splat4(0.f); part[o] = splat4(0.f); }
    TrunkOps cur, nxt;
    kload(0, cur);
    for (int T = 0; T < KT; ++T) {
        if (T + 1 < KT) kload(T + 1, nxt);
        f32x4 xn;
        for (int q = 0; q < 4; ++q) xn[q] = (valid && q < cur.kt.nv) ? fmaf((cur.x[q] - mu) * rstd, cur.gm[q], cur.bt[q]) : 0.f;
        for (int oo = 0; oo < PT; ++oo) part[oo] = mma_block(cur.wf[oo], xn, part[oo]);
        if ((T + 1) % TRUNK_GROUP == 0 || T + 1 == KT)
            for (int oo = 0; oo < PT; ++oo) { acc[oo] += part[oo]; part[oo] = splat4(0.f); }
        cur = nxt;
    }

    // the two 64-wide layers and the input side of the GRU
    const bool tanh = a.act_tanh != 0;
    f32x4 f1[PT], f2[PT];
    for (int t = 0; t < PT; ++t) f1[t] = trace_act4(acc[t] + bfrag_a(P + nw.off[IPLAN_AC_FC1_B], t), tanh);
    layer_norm_tiles<PT>(f1, P + nw.off[IPLAN_AC_LN1_W], P + nw.off[IPLAN_AC_LN1_B], nullptr, nullptr);
    for (int t = 0; t < PT; ++t)
        f2[t] = trace_act4(dense_tile_ga<PT>(P + nw.off[IPLAN_AC_FC2_W], PM, PM, 16 * t, f1, bfrag_a(P + nw.off[IPLAN_AC_FC2_B], t)), tanh);
    layer_norm_tiles<PT>(f2, P + nw.off[IPLAN_AC_LN2_W], P + nw.off[IPLAN_AC_LN2_B], nullptr, nullptr);
#ifdef TRUNK_GI_ROW
    float* girow = TRUNK_GI_ROW;
    for (int t = 0; t < 3 * PT; ++t)
        vstore_a(girow, valid, t, dense_tile_ga<PT>(P + nw.off[IPLAN_AC_WIH], PM, 3 * PM, 16 * t, f2, bfrag_a(P + nw.off[IPLAN_AC_BIH], t)));
#endif
