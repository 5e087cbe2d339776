// The statements of a saliency kernel's body (sal_body.h), included as text inside the kernel.  The including function provides
//   constexpr int MODE                     0 | 1 | 2 (sal_body.h)
//   const IplanAcSaliencyArgs& a           the row description
//   const IplanAcSaliencyLagArgs* x_       the lag arguments (MODE 0: never read)
//   SalShared sh                           __shared__
// (no include guard: one inclusion per kernel)
    const int lag = MODE == 2 ? x_->lag : 0;
    const int net = (int)blockIdx.y, which = a.which == 2 ? (int)blockIdx.z : a.which;
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const IplanAcFeatures& ft = a.feat;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int64_t rows = (int64_t)a.E * a.S;
    const int64_t tile = (int64_t)blockIdx.x * SAL_WAVES + w;
    if (tile * 16 >= rows) return;                                           // (whole wave; the kernel has no barrier)
    const int64_t r = tile * 16 + n;
    const bool valid = MODE == 2 ? (r < rows && r % a.S >= lag) : r < rows;
    const int64_t ec = valid ? r / a.S : 0, sc = valid ? r % a.S - lag : 0;  // (sc: the step whose inputs and entering state are read)
    const int64_t pr = ec * ft.T_phys + sc;
    const int64_t orow = (int64_t)net * rows + (valid ? r : 0);
    const float* src[3];
    for (int s = 0; s < 3; ++s) src[s] = ft.w[s] > 0 ? ft.src[s] + (int64_t)net * ft.s_net[s] + pr * ft.s_row[s] : nullptr;
    int last = -1;
    if (valid && ft.n_actions > 0) {
        if (ft.last_action) last = ft.last_action[(int64_t)net * ft.la_s_net + pr * ft.la_s_row];
        else if (ft.last_action64) last = (int)ft.last_action64[(int64_t)net * ft.la64_s_net + pr * ft.la64_s_row];
    }
    const KMap km = make_kmap(ft);                                           // (kfeat reads the one-hot widths from it)
    const SalMap sm = sal_make_map(ft);
    const int F = sm.NW + ft.n_actions + ft.n_id, KT = sm.KT;
    const bool tanh = a.act_tanh != 0;

    // ---- passes 1, 2: LayerNorm(F) statistics
    float sum = 0.f;
    for (int T = 0; T < KT; ++T) {
        const f32x4 x = kfeat(km, sal_ktile(sm, T), src, valid, last, net);
        sum += (x[0] + x[1]) + (x[2] + x[3]);
    }
    const float mu = group_sum(sum) / (float)F;
    float sq = 0.f;
    for (int T = 0; T < KT; ++T) {
        const KTile kt = sal_ktile(sm, T);
        const f32x4 x = kfeat(km, kt, src, valid, last, net);
        for (int q = 0; q < 4; ++q)
            if (q < kt.nv) { const float d = x[q] - mu; sq = fmaf(d, d, sq); }
    }
    const float rstd = 1.0f / sqrtf(group_sum(sq) / (float)F + 1e-5f);

    // ---- pass 3: fc1; operands from the fragment-major pack (iplan_ac_pack_fc1) or from the arena in place
    const float* __restrict__ pkw = which ? a.packed_critic : a.packed_actor;
    if (pkw) pkw += (int64_t)net * a.packed_s_net;
    const float* __restrict__ pkg = pkw ? pkw + (int64_t)KT * 1024 : nullptr;
    const float* __restrict__ pkb = pkw ? pkg + (int64_t)KT * 16 : nullptr;
    const float* fnw = P + nw.off[IPLAN_AC_FN_W];
    const float* fnb = P + nw.off[IPLAN_AC_FN_B];
    const float* W1 = P + nw.off[IPLAN_AC_FC1_W];
    f32x4 acc[ST], part[ST];
    for (int o = 0; o < ST; ++o) { acc[o] = splat4(0.f); part[o] = splat4(0.f); }
    for (int T = 0; T < KT; ++T) {
        const KTile kt = sal_ktile(sm, T);
        const f32x4 x = kfeat(km, kt, src, valid, last, net);
        f32x4 gm, bt, wf[ST];
        if (pkw) {
            gm = *reinterpret_cast<const f32x4*>(pkg + T * 16 + 4 * g);
            bt = *reinterpret_cast<const f32x4*>(pkb + T * 16 + 4 * g);
            for (int oo = 0; oo < ST; ++oo) wf[oo] = *reinterpret_cast<const f32x4*>(pkw + ((int64_t)(T * ST + oo) * 64 + l) * 4);
        } else {
            gm = kcols(kt, fnw);
            bt = kcols(kt, fnb);
            for (int oo = 0; oo < ST; ++oo) wf[oo] = kcols(kt, W1 + (int64_t)(16 * oo + n) * F);
        }
        f32x4 xn;
        for (int q = 0; q < 4; ++q) xn[q] = (valid && q < kt.nv) ? fmaf((x[q] - mu) * rstd, gm[q], bt[q]) : 0.f;
        for (int oo = 0; oo < ST; ++oo) part[oo] = mma_block(wf[oo], xn, part[oo]);
        if ((T + 1) % SAL_GROUP == 0 || T + 1 == KT)
            for (int oo = 0; oo < ST; ++oo) { acc[oo] += part[oo]; part[oo] = splat4(0.f); }
    }

    // ---- the 64-wide layers forward; a1, a2, hn are kept as the values the three LayerNorms normalise
    f32x4 a1[ST], a2[ST], f[ST];
    float mu1, rs1, mu2, rs2, mu3, rs3;
    for (int t = 0; t < ST; ++t) f[t] = a1[t] = sal_act4(acc[t] + bfrag_a(P + nw.off[IPLAN_AC_FC1_B], t), tanh);
    layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN1_W], P + nw.off[IPLAN_AC_LN1_B], &mu1, &rs1);
    for (int t = 0; t < ST; ++t)
        a2[t] = sal_act4(dense_tile_ga<ST>(P + nw.off[IPLAN_AC_FC2_W], SM, SM, 16 * t, f, bfrag_a(P + nw.off[IPLAN_AC_FC2_B], t)), tanh);
    for (int t = 0; t < ST; ++t) f[t] = a2[t];
    layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN2_W], P + nw.off[IPLAN_AC_LN2_B], &mu2, &rs2);
    float* act1 = which ? a.act1_critic : a.act1_actor;
    float* act2 = which ? a.act2_critic : a.act2_actor;
    if constexpr (MODE != 2)
        for (int t = 0; t < ST; ++t) {
            if (act1) vstore_a(act1 + orow * SM, valid, t, a1[t]);
            if (act2) vstore_a(act2 + orow * SM, valid, t, a2[t]);
        }

    // the GRU cell from the given state: gi = W_ih f + b_ih, gh = W_hh h + b_hh, the gates of wave_tile.h
    const float* hsrc = which ? a.h_critic : a.h_actor;
    const float* hrow = hsrc + (int64_t)net * a.hs_net + ec * a.hs_chain + sc * a.hs_step;
    f32x4 h[ST], gr[ST], gz[ST], gn[ST], ghn[ST], hn[ST];
    for (int t = 0; t < ST; ++t) h[t] = vload(hrow, valid, SM, t);
    for (int t = 0; t < ST; ++t) {
        f32x4 gi[3], gh[3];
        for (int k = 0; k < 3; ++k) {
            gi[k] = dense_tile_ga<ST>(P + nw.off[IPLAN_AC_WIH], SM, 3 * SM, k * SM + 16 * t, f, bfrag_a(P + nw.off[IPLAN_AC_BIH], k * ST + t));
            gh[k] = dense_tile_ga<ST>(P + nw.off[IPLAN_AC_WHH], SM, 3 * SM, k * SM + 16 * t, h, bfrag_a(P + nw.off[IPLAN_AC_BHH], k * ST + t));
        }
        const GruGates o = gru_gates(gi[0] + gh[0], gi[1] + gh[1], gi[2], gh[2], h[t]);
        gr[t] = o.r; gz[t] = o.z; gn[t] = o.n; ghn[t] = o.hn; hn[t] = o.h;
    }
    f32x4 d[ST];                                                             // d y / d h' (the GRU output before rnn.norm)
    if constexpr (MODE == 2) {
        const float* seed = (which ? x_->seed_critic : x_->seed_actor) + orow * x_->seed_s_row;
        for (int t = 0; t < ST; ++t) d[t] = vload_a(seed, valid, t);
    } else {
        for (int t = 0; t < ST; ++t) f[t] = hn[t];
        layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN3_W], P + nw.off[IPLAN_AC_LN3_B], &mu3, &rs3);
        const int n_out = nw.n_out;
        f32x4 lg = bfrag(P + nw.off[IPLAN_AC_HEAD_B], n_out, 0);
        for (int t = 0; t < ST; ++t) lg = mma_block(wfrag_a(P + nw.off[IPLAN_AC_HEAD_W], SM, n_out, 0, 16 * t), f[t], lg);

        // ---- y and d y / d logits (lane (n, g) holds outputs 4 g .. 4 g + 3 of row n)
        f32x4 dl = splat4(0.f);
        if (which == 1) {
            if (g == 0) dl[0] = 1.0f;
            if (valid && g == 0 && a.values) a.values[orow] = lg[0];
        } else {
            // the masked categorical of ac_categorical.h
            const int32_t* av = (a.avail && valid) ? a.avail + (int64_t)net * a.av_s_net + ec * a.av_s_chain + sc * a.av_s_step : nullptr;
            const MaskedCat c = masked_categorical(lg, av, g, n_out);
            int64_t want = a.target_all;
            if (a.target && valid) want = a.target[(int64_t)net * a.tg_s_net + ec * a.tg_s_chain + sc * a.tg_s_step];
            const int action = (want >= 0 && want < n_out) ? (int)want : c.cand;
            float sel = 0.f;
            for (int q = 0; q < 4; ++q) {
                const int idx = 4 * g + q;
                if (idx == action) sel += c.lp[q];
                if (idx < n_out && !((c.offm >> q) & 1)) dl[q] = (idx == action ? 1.0f : 0.0f) - c.pb[q];   // (no gradient into a masked logit)
            }
            sel = group_sum(sel);
            if (valid && g == 0) {
                if (a.logp) a.logp[orow] = sel;
                if (a.target_out) a.target_out[orow] = (int64_t)action;
            }
        }

        // ---- backward through the head and rnn.norm
        {
            const f32x4 dlt[1] = {dl};
            for (int t = 0; t < ST; ++t) d[t] = dense_tile_gt<1>(P + nw.off[IPLAN_AC_HEAD_W], SM, n_out, SM, 16 * t, dlt, splat4(0.f));
        }
        sal_ln_bwd(d, hn, mu3, rs3, P + nw.off[IPLAN_AC_LN3_W]);
    }
    // ---- backward through the 64-wide layers: d[] ends as delta = d y / d z1
    f32x4 dgi[3 * ST];                                                       // d y / d gi: r | z | n
    if constexpr (MODE == 0) {
        for (int t = 0; t < ST; ++t) {
            const GruGrads o = gru_gates_bwd(d[t], gr[t], gz[t], gn[t], ghn[t], h[t]);
            dgi[t] = o.dr; dgi[ST + t] = o.dz; dgi[2 * ST + t] = o.dni;
        }
    } else {
        // the link through the state, formed and stored here so that it is not live across passes 4-5:
        //   carry = d y / d h_prev = z * d y / d h' + W_hh^T [dr | dz | r * dn]
        f32x4 dgh[3 * ST], dhd[ST];                                          // d y / d gh: r | z | n; the direct path
        for (int t = 0; t < ST; ++t) {
            const GruGrads o = gru_gates_bwd(d[t], gr[t], gz[t], gn[t], ghn[t], h[t]);
            dgi[t] = dgh[t] = o.dr; dgi[ST + t] = dgh[ST + t] = o.dz; dgi[2 * ST + t] = o.dni;
            dgh[2 * ST + t] = o.dnh; dhd[t] = o.dh_direct;
        }
        float* carry = which ? x_->carry_critic : x_->carry_actor;
        if (carry)
            for (int t = 0; t < ST; ++t)
                vstore_a(carry + orow * x_->carry_s_row, valid, t, dhd[t] + sal_dense_t<3 * ST>(P + nw.off[IPLAN_AC_WHH], t, dgh));
    }
    for (int t = 0; t < ST; ++t) d[t] = sal_dense_t<3 * ST>(P + nw.off[IPLAN_AC_WIH], t, dgi);
    sal_ln_bwd(d, a2, mu2, rs2, P + nw.off[IPLAN_AC_LN2_W]);
    f32x4 dz[ST];
    for (int t = 0; t < ST; ++t) dz[t] = sal_dact4(d[t], a2[t], tanh);
    for (int t = 0; t < ST; ++t) d[t] = sal_dense_t<ST>(P + nw.off[IPLAN_AC_FC2_W], t, dz);
    sal_ln_bwd(d, a1, mu1, rs1, P + nw.off[IPLAN_AC_LN1_W]);
    for (int t = 0; t < ST; ++t) d[t] = sal_dact4(d[t], a1[t], tanh);

    // ---- passes 4, 5: fc1^T and the LayerNorm(F) backward
    auto ktile_bwd = [&](int T) {
        SalTile o;
        o.kt = sal_ktile(sm, T);
        o.x = kfeat(km, o.kt, src, valid, last, net);
        // A = W1^T: this lane's output row is entry m = n of the k-tile; its column of fc1.weight, and whether the entry exists
        f32x4 wt[ST];
        if (pkw) {
            const float* p = pkw + ((int64_t)T * ST * 64 + 4 * g + 16 * (n >> 2)) * 4 + (n & 3);
            for (int t = 0; t < ST; ++t)
                for (int q = 0; q < 4; ++q) wt[t][q] = as_global(p)[(t * 64 + q) * 4];
        } else {
            const KTile km_ = sal_ktile_at(sm, T, 4 * (n >> 2));
            const int qm = n & 3;
            const bool ok = qm < km_.nv;
            const int cm = qm == 0 ? km_.c[0] : (qm == 1 ? km_.c[1] : (qm == 2 ? km_.c[2] : km_.c[3]));
            const float* p = W1 + (ok ? cm : 0) + (int64_t)(4 * g) * F;
            for (int t = 0; t < ST; ++t)
                for (int q = 0; q < 4; ++q) wt[t][q] = keep_if(ok, as_global(p)[(int64_t)(16 * t + q) * F]);
        }
        f32x4 u = splat4(0.f);
        for (int t = 0; t < ST; ++t) u = mma_block(wt[t], d[t], u);
        const f32x4 gm = pkw ? *reinterpret_cast<const f32x4*>(pkg + T * 16 + 4 * g) : kcols(o.kt, fnw);
        for (int q = 0; q < 4; ++q) {
            o.xh[q] = (o.x[q] - mu) * rstd;
            o.gh[q] = gm[q] * u[q];
        }
        return o;
    };
    float s1 = 0.f, s2 = 0.f;
    for (int T = 0; T < KT; ++T) {
        const SalTile o = ktile_bwd(T);
        for (int q = 0; q < 4; ++q)
            if (valid && q < o.kt.nv) { s1 += o.gh[q]; s2 = fmaf(o.gh[q], o.xh[q], s2); }
    }
    const float m1 = group_sum(s1) / (float)F, m2 = group_sum(s2) / (float)F;

    float* ig = which ? a.input_grad_critic : a.input_grad_actor;
    float* ent = which ? a.entity_critic : a.entity_actor;
    const int n_src = (sm.w0 > 0) + (sm.w1 > 0) + (sm.w2 > 0);
    const int64_t grow = MODE == 0 ? orow : orow * x_->n_lags + x_->lag;      // the lag modes' results are [.., n_lags, ..]
    float* igrow = ig ? ig + grow * F : nullptr;
    float* entrow = ent ? ent + grow * ft.N * n_src * 2 : nullptr;
    const int b_kt0 = sm.kt00, b_kt1 = sm.kt01, b_kt2 = sm.kt02, b_w0 = sm.w0, b_w1 = sm.w1, b_w2 = sm.w2, b_len0 = sm.len0, b_len1 = sm.len1, b_len2 = sm.len2;
    float ax = 0.f, al = 0.f;                                                // the running sums of the entity being added (lanes g = 0)
    int ej = 0, ee = 0;                                                      // columns of it added so far; the entity
    for (int T = 0; T < KT; ++T) {
        const SalTile o = ktile_bwd(T);
        f32x4 dx;
        for (int q = 0; q < 4; ++q) dx[q] = (valid && q < o.kt.nv) ? (o.gh[q] - m1 - o.xh[q] * m2) * rstd : 0.f;
        if (igrow && valid)
            for (int q = 0; q < 4; ++q)
                if (q < o.kt.nv) igrow[o.kt.c[q]] = dx[q];
        const int s = o.kt.s;                                                // (uniform: the block depends on T alone)
        if (!entrow || s == 3) continue;
        f32x4 px, pl;
        for (int q = 0; q < 4; ++q) { px[q] = dx[q] * o.x[q]; pl[q] = fabsf(dx[q]); }
        *reinterpret_cast<f32x4*>(&sh.v[w][0][n][4 * g]) = px;
        *reinterpret_cast<f32x4*>(&sh.v[w][1][n][4 * g]) = pl;
        IPLAN_WAVE_SYNC();
        if (g == 0) {
            const int t0 = T - (s == 0 ? b_kt0 : (s == 1 ? b_kt1 : b_kt2));
            const int ws = s == 0 ? b_w0 : (s == 1 ? b_w1 : b_w2);
            const int ls = s == 0 ? b_len0 : (s == 1 ? b_len1 : b_len2);
            if (t0 == 0) { ax = al = 0.f; ej = ee = 0; }
            const int cnt = imin(16, ls - 16 * t0);
            const int si = s == 0 ? 0 : (s == 1 ? (b_w0 > 0) : (b_w0 > 0) + (b_w1 > 0));
            f32x4 vx[4], vl[4];
            for (int k = 0; k < 4; ++k) {
                vx[k] = *reinterpret_cast<const f32x4*>(&sh.v[w][0][n][4 * k]);
                vl[k] = *reinterpret_cast<const f32x4*>(&sh.v[w][1][n][4 * k]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i >= cnt) continue;
                ax += vx[i >> 2][i & 3];
                al += vl[i >> 2][i & 3];
                if (++ej == ws) {
                    if (valid) {
                        float* p = entrow + ((int64_t)ee * n_src + si) * 2;
                        p[0] = ax;
                        p[1] = al;
                    }
                    ax = al = 0.f;
                    ej = 0;
                    ++ee;
                }
            }
        }
        IPLAN_WAVE_SYNC();
    }
