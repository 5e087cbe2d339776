"""Per-piece timings of the hot path at BASELINE.json config 3 (E = 32, 5 agents x 55 entities), HIP events
around the host-level calls.  Usage: python scripts/microbench.py [piece ...]   (default: all)"""
import contextlib
import io
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iplan_amd import ops  # noqa: E402
from iplan_amd.config import default_args  # noqa: E402
from iplan_amd.harness import SyntheticLoop  # noqa: E402
from iplan_amd.nova.GAT_Net import gumbel_noise  # noqa: E402

E = int(os.environ.get("MB_ENVS", "32"))
args = default_args("highway", use_cuda=True, batch_size_run=E)
dev = torch.device("cuda")
loop = SyntheticLoop(args, E, seed=0, device=dev)
nA, N, d, Z, A = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim, args.attention_dim
want = set(sys.argv[1:])


def tm(name, fn, n=10, warm=2):
    if want and name.split(":")[0] not in want:
        return
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"{name:34s} gpu {e0.elapsed_time(e1) / n:9.3f} ms   wall {(time.perf_counter() - t0) / n * 1e3:9.3f} ms", flush=True)


hist = loop.obs_sets[0]["hist"][0].permute(1, 0, 2, 3)
lat = torch.softmax(torch.randn(nA, E, N, Z, device=dev), -1)
hid = torch.randn(nA, E, N, A, device=dev) * 0.1
noise = gumbel_noise((nA, E, N, N - 1, 2), dev)
out = torch.empty(nA, E, N, A, device=dev)
tm("gat_fwd", lambda: ops.gat_forward(loop.prediction.gat_arena, hist, lat, hid, noise, out=out), n=50)

window = loop.obs_sets[0]["hist"][0:10].permute(1, 2, 3, 0, 4).contiguous()
eh = torch.zeros(E, 1, nA, N, 32, device=dev)
lat_e = lat.permute(1, 0, 2, 3).contiguous()
tm("enc_fwd", lambda: loop.behavior.latent_update(window, eh, lat_e), n=50)

with contextlib.redirect_stdout(io.StringIO()):
    batch = loop.rollout()
tm("select_actions", lambda: loop.mac.select_actions_ippo(batch, 3, test_mode=False, as_numpy=False), n=50)
tm("rollout", lambda: loop.rollout(), n=2, warm=1)
if os.environ.get("MB_DEFER"):
    # the form the training cycle runs (harness.cycle): decoder weight gradients + optimiser step as ONE deferred iplan_wgrad call
    # on the side stream -- the PMC passes use it so that the per-kernel counters are those of the kernels bench.py times
    def beh_learn():
        loop.behavior.learn(batch, 0, defer_decoder=True)
        loop.behavior.join_decoder()
    tm("behavior_learn", beh_learn, n=3, warm=1)
else:
    tm("behavior_learn", lambda: loop.behavior.learn(batch, 0), n=3, warm=1)
tm("prediction_learn", lambda: loop.prediction.learn(batch, 0), n=5, warm=1)


def ppo():
    while not loop.learner.buffers[0].can_sample():
        loop.learner.insert_episode_batch(batch)
    with contextlib.redirect_stdout(io.StringIO()):
        loop.learner.train(0)


tm("ppo_train", ppo, n=2, warm=1)

if not want or "ac_train_parts" in want:
    # the pieces of one PPO epoch
    while not loop.learner.buffers[0].can_sample():
        loop.learner.insert_episode_batch(batch)
    L = loop.learner
    dd = L.store.data
    T = args.episode_limit
    acts = dd["actions"][..., 0]
    last = torch.cat([acts[:, :1], acts[:, :-1]], dim=1).to(torch.int32).contiguous()
    spec = L._feature_spec(T, T + 1, last)
    ha, hc = dd["rnn_states_actors"], dd["rnn_states_critics"]
    avail = dd["avail_actions"]
    rows = args.batch_size * T
    kw = dict(h_actor=ha, h_critic=hc, h_strides=(ha.stride(2), ha.stride(1)), avail=avail, avail_strides=(avail.stride(2), avail.stride(1)),
              mode=2, actions_in=dd["actions"], act_strides=(dd["actions"].stride(2), dd["actions"].stride(1)), n_actions=5, ksplit=1, want_h=False)
    want = set()
    tm("ac_fwd_train(infer)", lambda: ops.ac_forward(loop.mac.actor_arena, loop.mac.critic_arena, 2, spec, rows, nA, **kw), n=5)
    tm("ac_fwd_train(save)", lambda: ops.ac_forward(loop.mac.actor_arena, loop.mac.critic_arena, 2, spec, rows, nA, save=True, want_entropy=True, **kw), n=5)
    fo = ops.ac_forward(loop.mac.actor_arena, loop.mac.critic_arena, 2, spec, rows, nA, save=True, want_entropy=True, **kw)
    # what a PPO epoch launches: cached LayerNorm(F) statistics (mode 2) and the pre-packed fc1 operands
    lns = torch.empty(nA, args.batch_size * (T + 1), 2, device=dev)
    pk = loop.mac.fc1_pack.get(spec)
    ops.ac_forward(loop.mac.actor_arena, loop.mac.critic_arena, 2, spec, rows, nA, ln_stats=lns, ln_stats_mode=1, packed=pk, **kw)
    tm("ac_fwd_train(epoch form)", lambda: ops.ac_forward(loop.mac.actor_arena, loop.mac.critic_arena, 2, spec, rows, nA, save=True, want_entropy=True,
                                                          ln_stats=lns, ln_stats_mode=2, packed=pk, **kw), n=5)
    clk = torch.zeros(4, dtype=torch.int64, device=dev)
    for _ in range(2):
        ops.ac_forward(loop.mac.actor_arena, loop.mac.critic_arena, 2, spec, rows, nA, save=True, want_entropy=True, ln_stats=lns, ln_stats_mode=2,
                       packed=pk, phase_clocks=clk, **kw)
    torch.cuda.synchronize()
    cc = clk.cpu().double()
    print("ac_fwd (epoch form) phases of wave 0 of WG 0, x10 ns: stats, fc1 contraction, tail (2 row tiles) =", (cc[1:] - cc[:-1]).tolist())
    g1 = torch.randn(nA, rows, device=dev)
    tm("ac_backward(all)", lambda: ops.ac_backward(fo, loop.mac.actor_arena, loop.mac.critic_arena, g_logp=g1, g_entropy=-1e-6, g_values=g1), n=5)

if "predict" in set(sys.argv[1:]):
    # inference (iplan_predict, pred + metrics, targets read in place) against the training forward (iplan_pdec_fwd on gathered copies) at
    # the dense evaluation shape: every start step of every episode = E x (T - P - 1) samples per agent-net; then a whole evaluate()
    P, T = args.pred_length, args.episode_limit
    pol = loop.prediction
    history = batch["history"][:, :-1].float()
    n_t = T - P - 1
    S = E * n_t
    ei, ti = torch.arange(E).repeat_interleave(n_t), torch.arange(n_t).repeat(E)
    sE, sT, sA, sN, _ = history.stride()
    offset = (torch.arange(nA)[:, None] * sA + (ei * sE + ti * sT)[None, :]).to(torch.int64).to(dev)
    h0 = torch.randn(nA, S * N, A, device=dev) * 0.1
    weight = torch.ones(nA, S, device=dev)
    ag = torch.arange(nA)[:, None].expand(nA, S)
    x0 = history[ei[None], ti[None], ag].reshape(nA, S * N, d).contiguous()
    steps = ti[None, :, None] + 1 + torch.arange(P)[None, None, :]
    actual = history[ei[None, :, None], steps, ag[:, :, None]].permute(0, 1, 3, 2, 4).reshape(nA, S * N, P, d).contiguous()

    def run_predict():
        return ops.predict(pol.dec_arena, history, offset, sN, sT, h0, N, P, d, want_pred=True, want_metrics=True, weight=weight, presence_col=0,
                           checked=True)

    def run_pdec():
        return ops.pdec_forward(pol.dec_arena, x0, h0, actual, weight, N)

    a_, b_ = run_predict(), run_pdec()
    torch.cuda.synchronize()
    print("predict vs pdec_fwd predictions bit-equal:", torch.equal(a_["pred"], b_["pred"]), flush=True)
    del a_, b_

    def passes(fn, n_pass=7, n=5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n_pass):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / n)
        return out

    res = {"iplan_predict": [], "iplan_pdec_fwd": []}
    for _ in range(2):                                     # the two alternate, so a drift of the box hits both
        res["iplan_predict"] += passes(run_predict)
        res["iplan_pdec_fwd"] += passes(run_pdec)
    rows = nA * S * N
    must = {"iplan_predict": rows * 4 * (A + d + 2 * P * d), "iplan_pdec_fwd": rows * 4 * (A + d + 2 * P * d + P * 256)}
    for k, v in res.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"{k:16s} S={S} rows={rows} P={P}: median {med:.4f} ms  min {v[0]:.4f}  max {v[-1]:.4f}  spread {(v[-1] - v[0]) / med * 100:.1f} %  "
              f"bytes that must move {must[k] / 1e6:.1f} MB -> {must[k] / med / 1e9:.3f} TB/s = {must[k] / med / 1e9 / 8.0 * 100:.1f} % of the 8 TB/s peak", flush=True)
    nz = gumbel_noise((nA, 512, N, N - 1, 2), dev)
    g_x0 = history[ei[:512].to(dev), ti[:512].to(dev)].permute(1, 0, 2, 3)
    g_lat = batch["behavior_latent"][:, :-1].float()[ei[:512].to(dev), ti[:512].to(dev)].permute(1, 0, 2, 3)
    g_att = batch["attention_latent"][:, :-1].float()[ei[:512].to(dev), ti[:512].to(dev)].permute(1, 0, 2, 3)
    gat = sorted(passes(lambda: ops.gat_forward(pol.gat_arena, g_x0, g_lat, g_att, nz), n_pass=5, n=3))
    chunks = (S + 511) // 512
    print(f"gat_forward of one 512-sample chunk: median {gat[len(gat) // 2]:.3f} ms  (x {chunks} chunks = {gat[len(gat) // 2] * chunks:.2f} ms per evaluate)", flush=True)
    ev = sorted(passes(lambda: pol.evaluate(batch, defer=True), n_pass=5, n=1))
    print(f"Prediction_policy.evaluate (stride 1, {S} samples x {nA} agents, chunks of 512): median {ev[len(ev) // 2]:.2f} ms  min {ev[0]:.2f}  max {ev[-1]:.2f}",
          flush=True)

if "behavior_evaluate" in set(sys.argv[1:]):
    # behaviour-model inference (iplan_beh_eval, sums only: what evaluate() launches) against the training forward (iplan_beh_fwd with
    # drop_p = 0: records, carry buffers, encoder / decoder pieces on two streams) on the same episode views, alternating in one process;
    # then a whole Behavior_policy.evaluate (views, launch, window sums, one read-back) and the peak device memory each adds
    pol = loop.behavior
    v = pol.prepare_learn(batch)
    b_hist, b_mask, b_wn = v["hist"], v["mask"], v["win_norm"]
    Lw, T = args.max_history_len, args.episode_limit
    J = T - 1 - Lw
    tiles = (E * N + 15) // 16

    def run_eval():
        return ops.beh_eval(pol.enc_arena, pol.dec_arena, b_hist, b_mask, Lw, Z, args.soft_update_coef, args.thres_small_variation)

    def run_train_fwd():
        return ops.beh_forward(pol.enc_arena, pol.dec_arena, b_hist, b_mask, Lw, Z, args.soft_update_coef, args.thres_small_variation, 0.0,
                               seed=0, win_norm=b_wn)

    def bpasses(fn, n_pass=5, n=3):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n_pass):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / n)
        return out

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        level = torch.cuda.memory_allocated(dev)
        r = fn()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - level
        del r
        return extra

    res = {"iplan_beh_eval": [], "iplan_beh_fwd(drop_p=0)": []}
    for _ in range(2):                                     # the two alternate, so a drift of the box hits both
        res["iplan_beh_eval"] += bpasses(run_eval)
        res["iplan_beh_fwd(drop_p=0)"] += bpasses(run_train_fwd)
    mem = {"iplan_beh_eval": peak_extra(run_eval), "iplan_beh_fwd(drop_p=0)": peak_extra(run_train_fwd)}
    # 16-chain tile-steps x (encoder 104 + decoder 416) v_mfma_f32_16x16x4_f32 x 2048 FLOP; fp32 MFMA peak 157.3 TFLOP/s
    flop = nA * tiles * J * Lw * 520 * 2048.0
    for k, t in res.items():
        t = sorted(t)
        med = t[len(t) // 2]
        print(f"{k:24s} {nA} nets x {E * N} chains x {J} windows x {Lw} steps: median {med:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}  "
              f"spread {(t[-1] - t[0]) / med * 100:.1f} %  peak extra device memory {mem[k] / 2 ** 20:.1f} MiB"
              + (f"  {flop / med / 1e9:.1f} TFLOP/s = {flop / med / 1e9 / 157.3 * 100:.1f} % of the fp32 MFMA peak" if k == "iplan_beh_eval" else ""),
              flush=True)
    ev = sorted(bpasses(lambda: pol.evaluate(batch), n_pass=5, n=1))
    print(f"Behavior_policy.evaluate ({E} envs, no optional outputs): median {ev[len(ev) // 2]:.3f} ms  min {ev[0]:.3f}  max {ev[-1]:.3f}  "
          f"peak extra device memory {peak_extra(lambda: pol.evaluate(batch)) / 2 ** 20:.1f} MiB", flush=True)

if "latent_knockout" in set(sys.argv[1:]):
    # intent knock-out through time (iplan_enc_knockout through Behavior_policy.latent_knockout) against the route without it: one
    # latent_trace of the episode and one per occlusion interval on an explicitly modified copy, the differences and means in torch,
    # one read-back.  Q = 8 starts spread over the episode, D = 5, H = 20, want=("shift",); the two alternate in one process, a pair
    # of events around each call; median of 20 after 3 warm-up rounds.
    pol = loop.behavior
    k_hist = batch["history"][:, :-1].float().contiguous()                          # [E, T, nA, N, d]
    Lw = args.max_history_len
    T = k_hist.shape[1]
    J = T - 1 - Lw
    Qk, Dk, Hk = 8, 5, 20
    k_starts = sorted({round(i * (J - Hk) / (Qk - 1)) for i in range(Qk)})

    def run_knockout():
        r = pol.latent_knockout(k_hist, k_starts, duration=Dk, horizon=Hk, want=("shift",))
        return torch.stack([r["echo_shift"], r["echo_flip_rate"]]).cpu()

    def run_by_hand():
        base = pol.latent_trace(k_hist)                                                     # [E, J, nA, N, Z]
        rows = []
        for s in k_starts:
            c = k_hist.clone()
            c[:, s:s + Dk] = 0.0
            ko = pol.latent_trace(c)[:, s:s + Hk]
            ref = base[:, s:s + Hk]
            shift = (ko - ref).square().sum(-1).sqrt().double()                             # [E, H, nA, N]
            flip = (ko.argmax(-1) != ref.argmax(-1)).double()
            seen = (k_hist[:, s:s + Dk, :, :, 0] != 0).any(dim=1)[:, None].double()         # [E, 1, nA, N]
            cnt = seen.sum(dim=(0, 3)).clamp(min=1.0)                                       # [1, nA]
            rows.append(torch.stack([(shift * seen).sum(dim=(0, 3)) / cnt, (flip * seen).sum(dim=(0, 3)) / cnt]))
        return torch.stack(rows).cpu()

    a_new, a_old = run_knockout(), run_by_hand()                                            # [2, nA, Q, H] and [Q, 2, H, nA]
    print("largest difference of the two routes' echo_shift:", float((a_new[0] - a_old[:, 0].permute(2, 0, 1)).abs().max()), flush=True)
    times = {"latent_knockout": [], "latent_trace x (1 + Q) + torch": []}
    for rnd in range(23):
        for name, fn in (("latent_knockout", run_knockout), ("latent_trace x (1 + Q) + torch", run_by_hand)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd >= 3:
                times[name].append(e0.elapsed_time(e1))
    Jn = min(J, max(k_starts) + Hk)
    print(f"shape: {nA} nets x {E} envs x {N} entities, T = {T}, L = {Lw}, starts = {k_starts}, D = {Dk}, H = {Hk}; "
          f"workspace {4 * nA * E * N * Jn * 32 / 2 ** 20:.1f} MiB (he_j of {Jn} windows)", flush=True)
    for name, t in times.items():
        t = sorted(t)
        print(f"{name:32s} median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}  ({len(t)} rounds after 3 warm-up rounds)", flush=True)

if "forecast_knockout" in set(sys.argv[1:]):
    # forecasts under occlusion through time (iplan_predict_knockout through attention_knockout_trace(forecast=True)) against the route
    # without it: attention_knockout_trace(want=("latent_ko",)) under the same max_workspace_mb, ops.predict on it in chunks of
    # environments, the differences and the masked float64 sums in torch, one read-back.  55 entities all knocked, start = 30, D = 1,
    # H = 20, deterministic; the two alternate in one process, a pair of events around each call; median of 20 after 3 warm-up rounds.
    from iplan_amd import synth
    pol = loop.prediction
    P = args.pred_length
    S_f, start_f, D_f, H_f, mb_f, pos_f = 50, 30, 1, 20, 256, (1, 2)
    gen = torch.Generator().manual_seed(5)
    f_hist = synth.make_history(gen, (E, S_f, nA), N, d, presence_p=0.7).to(dev)
    f_lat = torch.softmax(torch.randn(E, S_f, nA, N, Z, generator=gen), -1).to(dev)
    f_hid = (torch.randn(E, nA, N, A, generator=gen) * 0.1).to(dev)
    f_src = f_hist.permute(2, 0, 1, 3, 4)
    f_s = f_src.stride()
    f_off = (torch.arange(nA)[:, None, None] * f_s[0] + torch.arange(E)[None, :, None] * f_s[1] +
             (start_f + torch.arange(H_f))[None, None, :] * f_s[2]).to(torch.int64).to(dev)      # [nA, E, H]

    def run_new(want=("shift",), mb=mb_f):
        return pol.attention_knockout_trace(f_hist, f_lat, f_hid, start=start_f, duration=D_f, horizon=H_f, forecast=True, pos=pos_f, want=want,
                                            max_workspace_mb=mb)

    def run_by_hand(ec=4):
        r = pol.attention_knockout_trace(f_hist, f_lat, f_hid, start=start_f, duration=D_f, horizon=H_f, want=("latent_ko",), max_workspace_mb=mb_f)
        lk = r["latent_ko"].permute(2, 0, 3, 1, 4, 5)                                       # [nA, E, J, H, N, A]
        Jn = lk.shape[2]
        pb = ops.predict(pol.dec_arena, f_src, f_off.reshape(nA, E * H_f).contiguous(), f_s[3], 0,
                         r["latent"].permute(2, 0, 1, 3, 4).reshape(nA, E * H_f * N, A).contiguous(), N, P, d, checked=True)["pred"].view(nA, E, H_f, N, P, d)
        fsh = torch.empty(nA, E, Jn, H_f, N, P, device=dev)
        for e0 in range(0, E, ec):
            e1 = min(E, e0 + ec)
            off = f_off[:, e0:e1, None].expand(nA, e1 - e0, Jn, H_f).reshape(nA, -1).contiguous()
            pk = ops.predict(pol.dec_arena, f_src, off, f_s[3], 0, lk[:, e0:e1].reshape(nA, (e1 - e0) * Jn * H_f * N, A).contiguous(), N, P, d,
                             checked=True)["pred"].view(nA, e1 - e0, Jn, H_f, N, P, d)
            acc = None
            for c in pos_f:
                df = pk[..., c] - pb[:, e0:e1, None, ..., c]
                acc = df * df if acc is None else acc + df * df
            fsh[:, e0:e1] = acc.sqrt()
        present = f_src[:, :, start_f:start_f + H_f, :, 0] != 0                             # [nA, E, H, N]
        seen = present[:, :, :D_f].any(dim=2)                                               # [nA, E, J = N]
        own = torch.eye(N, dtype=torch.bool, device=dev)
        count = present[:, :, None] & seen[:, :, :, None, None]
        parts = []
        for pick in (~own, own):
            m = count & pick[None, None, :, None, :]
            parts += [torch.where(m[..., None], fsh, 0.0).sum(dim=(2, 4), dtype=torch.float64), m.sum(dim=(2, 4), dtype=torch.float64)[..., None].expand(nA, E, H_f, P)]
        host = torch.stack(parts).cpu().numpy().sum(axis=2)                                 # the one read-back; [4, nA, H, P]
        return fsh, host

    r_new, (fsh_old, host_old) = run_new(), run_by_hand()
    fsh_new = r_new["forecast_shift"].permute(2, 0, 4, 1, 3, 5)
    print("the two routes' forecast_shift bit-equal:", bool(torch.equal(fsh_new.contiguous().view(torch.int32), fsh_old.view(torch.int32))),
          " largest:", float(fsh_new.max()), " in echo steps:", float(fsh_new[:, :, :, D_f:].max()), flush=True)
    import numpy as np
    with np.errstate(divide="ignore", invalid="ignore"):
        old_mean = host_old[0] / host_old[1]
    print("largest difference of the two routes' forecast_summary[..., 0]:", float(np.nanmax(np.abs(old_mean - r_new["forecast_summary"][..., 0]))), flush=True)
    # (the last two rows say where the time goes: without the latent shift and its summary, and without chunking)
    routes = {"attention_knockout_trace(forecast=True)": run_new, "latent_ko + ops.predict + torch": run_by_hand,
              "forecast=True, want=()": lambda: run_new(want=()), "forecast=True, want=(), 4096 MB": lambda: run_new(want=(), mb=4096)}
    times = {name: [] for name in routes}
    for rnd in range(23):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd >= 3:
                times[name].append(e0.elapsed_time(e1))
    # the launches' shares: events around each op's launches in one more call
    spans, orig = {}, {k: getattr(ops, k) for k in ("gat_trace", "gat_knockout_trace", "predict", "predict_knockout")}

    def timed(k):
        def call(*a_, **kw_):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = orig[k](*a_, **kw_)
            e1.record()
            spans.setdefault(k, []).append((e0, e1))
            return res
        return call
    for k in orig:
        setattr(ops, k, timed(k))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run_new()
    e1.record()
    torch.cuda.synchronize()
    for k in orig:
        setattr(ops, k, orig[k])
    print(f"one call of {e0.elapsed_time(e1):.3f} ms: " + ", ".join(f"{k} {len(v)} launches {sum(a_.elapsed_time(b_) for a_, b_ in v):.3f} ms" for k, v in spans.items()), flush=True)
    per_env = 4 * nA * H_f * (2 * N * (N - 1) + N * A + N * P * d)
    per_job = 4 * nA * H_f * (N + N * A + N * P)
    jc = min(N, (mb_f * 2 ** 20 - per_env) // per_job)
    ec = min(E, mb_f * 2 ** 20 // (per_env + jc * per_job))
    print(f"shape: {nA} nets x {E} envs x {N} entities, S = {S_f}, start = {start_f}, D = {D_f}, H = {H_f}, P = {P}; chunks of {ec} envs x {jc} jobs, "
          f"latent_ko workspace {4 * nA * ec * jc * H_f * N * A / 2 ** 20:.1f} MiB per chunk (the whole latent_ko: {4 * nA * E * N * H_f * N * A / 2 ** 20:.1f} MiB)", flush=True)
    for name, t in times.items():
        t = sorted(t)
        print(f"{name:42s} median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}  ({len(t)} rounds after 3 warm-up rounds)", flush=True)

if "gat_phases12" in set(sys.argv[1:]):           # libraries built with -DGAT_P3_CLOCKS only
    clk = torch.zeros(nA * E, 12, dtype=torch.int64, device=dev)
    ops.gat_forward(loop.prediction.gat_arena, hist, lat, hid, noise, out=out, phase_clocks=clk)
    torch.cuda.synchronize()
    c = clk.cpu().double()
    seq = c[:, [0, 1, 2, 5, 6, 7, 8, 9, 3, 4]]
    print("gat clocks x10 ns, mean per WG: entry->p1->p2->[noise issued]->[score GEMM]->[softmax]->[gate]->[aggregate]->barrier->p4:",
          (seq[:, 1:] - seq[:, :-1]).mean(0).tolist())

if "gat_bwd_phases" in set(sys.argv[1:]):     # training-form GAT (Prediction_policy.learn's shape: 64 sampled scenes per net)
    S = 64
    ar = loop.prediction.gat_arena
    ob = torch.rand(nA, S, N, hist.shape[-1], device=dev) * 2 - 1
    la = torch.rand(nA, S, N, lat.shape[-1], device=dev)
    hi = torch.randn(nA, S, N, 32, device=dev) * 0.1
    from iplan_amd.nova.GAT_Net import gumbel_noise
    nz = gumbel_noise((nA, S, N, N - 1, 2), dev)
    go = torch.randn(nA, S, N, 32, device=dev)

    def fb(clk=None):
        o, saved = ops.gat_forward(ar, ob, la, hi, nz, save=True)
        ops.gat_backward(ar, saved, go, phase_clocks=clk)
    tm("gat_fwd(save)+bwd+wgrad S=64", fb, n=5)
    tm("gat_fwd(save) S=64", lambda: ops.gat_forward(ar, ob, la, hi, nz, save=True), n=5)
    clk = torch.zeros(16, dtype=torch.int64, device=dev)
    fb(clk)
    torch.cuda.synchronize()
    c = clk.cpu().double()[8:15]
    print("gat_bwd phases of WG 0, x10 ns: A cell', B attention', C dk dv, D pair-GRU BPTT, E gather, F projections' =", (c[1:] - c[:-1]).tolist())

if "gat_phases" in set(sys.argv[1:]):
    clk = torch.zeros(nA * E, 5, dtype=torch.int64, device=dev)
    ops.gat_forward(loop.prediction.gat_arena, hist, lat, hid, noise, out=out, phase_clocks=clk)
    torch.cuda.synchronize()
    c = clk.cpu().double()
    d = (c[:, 1:] - c[:, :-1])
    print("gat phases (wall_clock64 ticks, 100 MHz => x10 ns): mean per WG", d.mean(0).tolist(), "max", d.max(0).values.tolist())
    print("kernel span ticks:", float(c[:, 4].max() - c[:, 0].min()), "first-start spread", float(c[:, 0].max() - c[:, 0].min()))

if "ac_phases" in set(sys.argv[1:]):
    clk = torch.zeros(4, dtype=torch.int64, device=dev)
    for _ in range(3):
        loop.mac.select_actions_ippo(batch, 3, test_mode=False, as_numpy=False, phase_clocks=clk)
    torch.cuda.synchronize()
    c = clk.cpu().double()
    print("ac_fwd (rollout) phases of WG 0, x10 ns: stats, contraction, tail =", (c[1:] - c[:-1]).tolist())

if "defer_overlap" in set(sys.argv[1:]):
    # critical path of Behavior_policy.learn with the decoder update in line / deferred, and the rollout that follows it
    def seq(defer, n=4):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tl = tr = 0.0
        for it in range(n + 1):
            torch.cuda.synchronize()
            ev[0].record()
            loop.behavior.learn(batch, 0, **({"defer_decoder": True} if defer else {}))
            ev[1].record()
            loop.rollout()
            ev[2].record()
            torch.cuda.synchronize()
            if it:
                tl += ev[0].elapsed_time(ev[1]) / n
                tr += ev[1].elapsed_time(ev[2]) / n
        return tl, tr
    work = torch.cuda.Stream(dev)          # (CU-masked streams are blocking streams: keep off the legacy default stream)
    for defer in (False, True, True):
        with torch.cuda.stream(work):
            tl, tr = seq(defer)
        print(f"defer_decoder={defer}: learn (main stream) {tl:.2f} ms, following rollout {tr:.2f} ms, sum {tl + tr:.2f} ms")

if "masked_wgrad" in set(sys.argv[1:]):
    # the deferred decoder update alone (nothing else on the GPU) on streams restricted to k CUs
    from iplan_amd.streams import masked_stream
    for k in (0, 128, 96, 64):
        loop.behavior._dec_stream = masked_stream(dev, k) if k else torch.cuda.Stream(dev)
        ts = []
        for it in range(3):
            loop.behavior.join_decoder()
            torch.cuda.synchronize()
            loop.behavior.learn(batch, 0, defer_decoder=True)
            torch.cuda.current_stream().synchronize()
            t0 = time.perf_counter()
            loop.behavior._dec_stream.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"deferred decoder update on {k or 256} CUs: {min(ts[1:]):.2f} ms after learn() returned (host clock)")

if "policy_trace" in set(sys.argv[1:]):
    # policy inspection (iplan_ac_trace: row-parallel trunk + one walk, both nets of every agent) against the only way the same numbers could
    # be had before it: S successive rollout-shaped ops.ac_forward(mode=2) launches of E rows with the state fed forward -- on the first S
    # steps of a rollout's own batch, alternating in one process; then the trace's two phases on their own
    S = int(os.environ.get("MB_TRACE_STEPS", "89"))
    mac = loop.mac
    D = batch.data
    T1 = D["history"].shape[1]
    n_act = args.n_actions
    acts = D["actions"][..., 0]                                                            # [E, T1, nA]
    last = torch.cat([torch.full_like(acts[:, :1], -1), acts[:, :-1]], 1)
    avail = D["avail_actions"]
    srcs = [(D[k][:, :S], w, D[k].stride(2), D[k].stride(1)) for k, w in mac._widths()]
    spec = ops.AcFeatureSpec(N, srcs, n_actions=n_act, last_action=last[:, :S], la_strides=(last.stride(2), last.stride(1)), n_id=nA, T=S, T_phys=T1)
    ha0, hc0 = D["rnn_states_actors"][:, 0], D["rnn_states_critics"][:, 0]
    kw = dict(hidden0_actor=ha0, hidden0_critic=hc0, h_strides=(ha0.stride(1), ha0.stride(0)), avail=avail[:, :S], avail_strides=(avail.stride(2), avail.stride(1)),
              actions_in=acts[:, :S], act_strides=(acts.stride(2), acts.stride(1)), n_actions=n_act)

    def run_trace():
        return ops.policy_trace(mac.actor_arena, mac.critic_arena, 2, spec, E, S, nA, packed=mac.fc1_pack.get(spec), **kw)

    step_specs = []
    for s in range(S):
        views = [(D[k][:, s], w, D[k].stride(2), D[k].stride(0)) for k, w in mac._widths()]
        la = last[:, s]
        step_specs.append(ops.AcFeatureSpec(N, views, n_actions=n_act, last_action=la, la_strides=(la.stride(1), la.stride(0)), n_id=nA, T=E, T_phys=E))

    def run_steps():
        ha, hc, hs = ha0, hc0, (ha0.stride(1), ha0.stride(0))
        outs = []
        for s in range(S):
            av, ac = avail[:, s], acts[:, s]
            o = ops.ac_forward(mac.actor_arena, mac.critic_arena, 2, step_specs[s], E, nA, h_actor=ha, h_critic=hc, h_strides=hs, avail=av,
                               avail_strides=(av.stride(1), av.stride(0)), mode=2, actions_in=ac, act_strides=(ac.stride(1), ac.stride(0)), n_actions=n_act,
                               want_probs=True, want_entropy=True, packed=mac.fc1_pack.get(step_specs[s], fold=True))
            ha, hc, hs = o["h_actor"], o["h_critic"], (E * 64, 64)
            outs.append(o)
        return outs

    a_, b_ = run_trace(), run_steps()
    torch.cuda.synchronize()
    for k in ("values", "logp"):
        ref = torch.stack([o[k] for o in b_], -1)
        print(f"policy_trace vs {S} ac_forward steps, {k}: max |difference| {(a_[k] - ref).abs().max().item():.3g} (scale {ref.abs().max().item():.3g})", flush=True)
    del a_, b_

    def passes(fn, n_pass=5, n=3):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(n_pass):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / n)
        return out

    lib = ops._lib(None)
    targs, tres, tkeep = ops.policy_trace_args(mac.actor_arena, mac.critic_arena, 2, spec, E, S, nA, packed=mac.fc1_pack.get(spec), **kw)
    stream = torch.cuda.current_stream().cuda_stream

    def run_phase(p):
        targs.phases = p
        lib.call("iplan_ac_trace", targs, stream)

    res = {"policy_trace": [], "ac_forward x S": [], "trace phase 1 (trunk)": [], "trace phase 2 (walk)": []}
    for _ in range(2):                                     # the candidates alternate, so a drift of the box hits all of them
        res["policy_trace"] += passes(run_trace)
        res["ac_forward x S"] += passes(run_steps)
        res["trace phase 1 (trunk)"] += passes(lambda: run_phase(1))
        res["trace phase 2 (walk)"] += passes(lambda: run_phase(2))
    for k, v in res.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"{k:24s} E={E} S={S} nA={nA} both nets: median {med:.4f} ms  min {v[0]:.4f}  max {v[-1]:.4f}  spread {(v[-1] - v[0]) / med * 100:.1f} %", flush=True)
