"""TEST INFRASTRUCTURE: trajectory-prediction inference (csrc/predict.hip, ops.predict, Prediction_policy.predict / evaluate) on
whatever library is active -- the host emulator in tests/test_emu_predict.py, the gfx950 build in tests/test_gpu_predict.py.

References: oracle.prediction_decoder_forward (no drop masks) and oracle.gat_forward in fp64, the metric sums from plain fp64 torch.
Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor (``_grad_err``), bound = max(1e-5, 1.5 x the fp32
oracle's own error against fp64), the fp32 error computed beside every reference; a metric sum is compared as sum / count.
The checks never touch ``L.use_library_for_tests``: the caller decides which library is active.  Each returns the worst errors it saw."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5

# (S, N, P, d, n_nets): rows S * N in {2, 15, 16, 17, 65} -- below, at and one past a wave's 16 rows, more than one block
# (65 rows = 5 tiles) --, every P and d with every tile raggedness at least once, one net and five
KERNEL_CASES = [
    (1, 2, 1, 4, 1), (1, 2, 5, 5, 5), (3, 5, 5, 5, 1), (3, 5, 12, 16, 5), (1, 16, 1, 5, 5), (1, 16, 12, 4, 1),
    (1, 17, 5, 16, 1), (1, 17, 1, 4, 5), (5, 13, 5, 5, 5), (5, 13, 12, 4, 1), (5, 13, 1, 16, 5),
]


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


class Case:
    """random decoder parameters, random h0, and a history buffer [time, net, entity, feature] whose entity, net and step
    strides are all larger than the packed ones; the samples' start steps are drawn with replacement from fewer steps than
    there are samples would need to be disjoint, so they are non-monotone and their windows overlap"""

    def __init__(self, S, N, P, d, n_nets, device, seed=0, presence_p=0.7):
        from iplan_amd.arena import ParamArena
        from iplan_amd.nova.prediction_net import Prediction_Decoder
        self.S, self.N, self.P, self.d, self.n_nets, self.device = S, N, P, d, n_nets, device
        torch.manual_seed(1000 * S + 100 * N + 10 * P + d + n_nets + seed)
        self.mods = [Prediction_Decoder(input_size=d, hidden_size=32, output_size=d, num_layers=1, pred_length=P,
                                        teacher_forcing_ratio=0, dropout=0.0) for _ in range(n_nets)]
        self.params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.mods]
        self.arena = ParamArena(self.mods, device)
        gen = torch.Generator().manual_seed(seed + S + N + P + d)
        self.ent_stride = d + 3
        self.net_stride = N * self.ent_stride + 2
        self.step_stride = n_nets * self.net_stride + 5
        self.T = max(2, (S + 1) // 2) + P + 1
        buf = torch.rand(self.T * self.step_stride + 7, generator=gen) * 2 - 1
        self.start = torch.randint(0, self.T - P - 1 + 1, (n_nets, S), generator=gen)
        if S >= 3:
            self.start[:, 0], self.start[:, 1], self.start[:, 2] = self.start[:, 0].clamp_min(1), 0, self.start[:, 0].clamp_min(1)
        self.offset = (3 + self.start * self.step_stride + torch.arange(n_nets)[:, None] * self.net_stride).to(torch.int64)
        # presence column 0 in {0, 1}
        rows = self._row_index(torch.arange(self.T)[:, None, None], torch.arange(n_nets)[None, :, None], torch.arange(N)[None, None, :])
        buf[rows] = (torch.rand(rows.shape, generator=gen) < presence_p).float()
        self.buf = buf
        self.h0 = torch.randn(n_nets, S * N, 32, generator=gen) * 0.5
        self.weight = torch.randint(0, 4, (n_nets, S), generator=gen).float() * 0.5           # 0, 0.5, 1, 1.5: sums are exact in fp32
        self.upload()

    def _row_index(self, t, n, i):
        return 3 + t * self.step_stride + n * self.net_stride + i * self.ent_stride

    def upload(self):
        dev = self.device
        self.d_buf, self.d_off, self.d_h0, self.d_w = self.buf.to(dev), self.offset.to(dev), self.h0.to(dev), self.weight.to(dev)

    def gather(self, dtype=torch.float32):
        """(x0 [n, S, N, d], target [n, S, N, P, d]) as the kernel must see them"""
        n, i, c = torch.arange(self.n_nets)[:, None, None, None], torch.arange(self.N)[None, None, :, None], torch.arange(self.d)
        t = self.start[:, :, None, None]
        x0 = self.buf[self._row_index(t, n, i) + c]
        tp = self.start[:, :, None, None, None] + 1 + torch.arange(self.P)[None, None, None, :, None]
        tg = self.buf[self._row_index(tp, n[..., None], i[..., None]) + c]
        return x0.to(dtype), tg.to(dtype)

    def run(self, pred=True, metrics=True, weight=True, presence_col=0, pos=(1, 2), target_none=False, checked=False):
        out = ops.predict(self.arena, self.d_buf, self.d_off, self.ent_stride, self.step_stride, self.d_h0, self.N, self.P, self.d,
                          want_pred=pred, want_metrics=metrics, target=None if (target_none or not metrics) else self.d_buf,
                          weight=self.d_w if weight else None, presence_col=presence_col, pos=pos, checked=checked)
        _sync(self.device)
        return out

    def reference(self, dtype, weight=True, presence_col=0, pos=(1, 2)):
        """(pred [n, S*N, P, d], sums [n, P, 3]) in ``dtype``"""
        x0, tg = self.gather(dtype)
        S, N, P, d = self.S, self.N, self.P, self.d
        preds, sums = [], []
        for n in range(self.n_nets):
            p = {k: v.to(dtype) for k, v in self.params[n].items()}
            pr = O.prediction_decoder_forward(p, x0[n].reshape(S, N, 1, d), self.h0[n].to(dtype), P)          # [S, N, P, d]
            delta = tg[n] - pr
            dist = (delta[..., list(pos)] ** 2).sum(-1).sqrt()
            l1 = delta.abs().sum(-1)
            w = (self.weight[n].to(dtype) if weight else torch.ones(S, dtype=dtype))[:, None, None].expand(S, N, P)
            if presence_col >= 0:
                w = w * (x0[n][..., presence_col] != 0).to(dtype)[:, :, None] * (tg[n][..., presence_col] != 0).to(dtype)
            preds.append(pr.reshape(S * N, P, d))
            sums.append(torch.stack([(w * dist).sum((0, 1)), (w * l1).sum((0, 1)), w.sum((0, 1))], -1))
        return torch.stack(preds), torch.stack(sums)


def _means(sums):
    """[n, P, 2]: the two error sums divided by their count (0 where nothing counts)"""
    c = sums[..., 2:3].double()
    return torch.where(c > 0, sums[..., :2].double() / c.clamp_min(1e-30), torch.zeros_like(sums[..., :2].double()))


def assert_vs_fp64(case, out, worst, what, **ref_kw):
    p64, s64 = case.reference(torch.float64, **ref_kw)
    p32, s32 = case.reference(torch.float32, **ref_kw)
    for n in range(case.n_nets):
        if out["pred"] is not None:
            e32, err = _grad_err(p32[n], p64[n]), _grad_err(out["pred"][n], p64[n])
            print(what, "net", n, "pred err", err, "e32", e32)
            _worse(worst, "pred", err)
            _worse(worst, "pred_e32", e32)
            assert err <= _bound(e32), (what, "pred", n, err, e32)
        if out["metrics"] is not None:
            got = out["metrics"][n].cpu()
            cerr = _grad_err(got[:, 2], s64[n][:, 2]) if s64[n][:, 2].abs().max() > 0 else float(got[:, 2].abs().max())
            print(what, "net", n, "count err", cerr)
            _worse(worst, "count", cerr)
            assert cerr <= TOL, (what, "count", n, cerr)
            if s64[n][:, 2].abs().max() == 0:
                assert torch.equal(got, torch.zeros_like(got)), (what, "sums of zero weights", n)
                continue
            for k, name in ((0, "displacement"), (1, "l1")):
                m64, m32, mg = _means(s64[n])[:, k], _means(s32[n])[:, k], _means(got)[:, k]
                e32, err = _grad_err(m32, m64), _grad_err(mg, m64)
                print(what, "net", n, name, "err", err, "e32", e32)
                _worse(worst, name, err)
                _worse(worst, name + "_e32", e32)
                assert err <= _bound(e32), (what, name, n, err, e32)


# ------------------------------------------------------------------------------------------------ the kernel alone
def check_kernel(device, S, N, P, d, n_nets):
    """pred and the three sums against fp64, pred + metrics in one launch"""
    case = Case(S, N, P, d, n_nets, device)
    worst = {}
    pos = (1, 2) if d > 4 else (2, 3)
    assert_vs_fp64(case, case.run(pos=pos), worst, (S, N, P, d, n_nets), pos=pos)
    return worst


def check_optional_operands(device, S=3, N=7, P=4, d=5, n_nets=2):
    """every optional operand with its mate present and absent: pred null, metrics null (no target: its pointer is 0), weights
    null, presence_col = -1.  What a launch does produce does not depend on what else it was asked for (bitwise)."""
    case = Case(S, N, P, d, n_nets, device, seed=5)
    worst = {}
    both = case.run()
    assert_vs_fp64(case, both, worst, "pred + metrics")
    only_pred = case.run(metrics=False, target_none=True)
    assert only_pred["metrics"] is None and only_pred["_args"].target is None and only_pred["_args"].metrics is None
    assert_vs_fp64(case, only_pred, worst, "pred only")
    assert torch.equal(only_pred["pred"], both["pred"])
    only_metrics = case.run(pred=False)
    assert only_metrics["pred"] is None and only_metrics["_args"].pred is None
    assert_vs_fp64(case, only_metrics, worst, "metrics only")
    assert torch.equal(only_metrics["metrics"], both["metrics"])
    for weight in (True, False):
        for pc in (0, -1):
            kw = dict(weight=weight, presence_col=pc)
            out = case.run(**kw)
            assert_vs_fp64(case, out, worst, ("weight", weight, "presence_col", pc), **kw)
            assert torch.equal(out["pred"], both["pred"])
            if not weight and pc < 0:                         # every row counts at every step
                assert torch.equal(out["metrics"][..., 2].cpu(), torch.full((n_nets, P), float(S * N)))
    # metrics without a target, and a launch that asks for nothing, are argument errors, not launches
    a = both["_args"]
    saved = a.target
    a.target = None
    try:
        ops._lib(None).call("iplan_predict", a)
        raise AssertionError("metrics without a target was accepted")
    except L.IplanError:
        pass
    a.target = saved
    return worst


def check_sentinel(device, S, N, P, d, n_nets):
    """pred and metrics (and the scratch partials) inside buffers pre-filled with a sentinel: every float the launch does not own
    comes back unchanged -- the padding lanes of a ragged last tile write nothing"""
    case = Case(S, N, P, d, n_nets, device, seed=9)
    ref = case.run()
    a = ref["_args"]
    pad = 64
    tiles = (S * N + 15) // 16
    sizes = dict(pred=n_nets * S * N * P * d, metrics=n_nets * P * 3, part=n_nets * P * 3 * tiles)
    bufs, sentinels = {}, {}
    for k, n in sizes.items():
        idx = torch.arange(n + 2 * pad, dtype=torch.float32)
        sentinels[k] = 0.5 + (idx % 1021) / 1024.0
        bufs[k] = sentinels[k].clone().to(device)
        setattr(a, k, bufs[k].data_ptr() + 4 * pad)
    ops._lib(None).call("iplan_predict", a, L.current_stream(device))
    _sync(device)
    for k, n in sizes.items():
        got = bufs[k].cpu()
        assert torch.equal(got[:pad].view(torch.int32), sentinels[k][:pad].view(torch.int32)), (k, "floats in front were written")
        assert torch.equal(got[pad + n:].view(torch.int32), sentinels[k][pad + n:].view(torch.int32)), (k, "floats behind were written")
    assert torch.equal(bufs["pred"][pad:pad + sizes["pred"]].view_as(ref["pred"]), ref["pred"])
    assert torch.equal(bufs["metrics"][pad:pad + sizes["metrics"]].view_as(ref["metrics"]), ref["metrics"])
    # every owned float of pred was written (the sentinel is never a prediction: compare with a second, shifted sentinel)
    others = {k: (sentinels[k] + 0.25).to(device) for k in ("pred", "metrics")}
    for k in others:
        setattr(a, k, others[k].data_ptr() + 4 * pad)
    ops._lib(None).call("iplan_predict", a, L.current_stream(device))
    _sync(device)
    for k in others:
        assert torch.equal(others[k][pad:pad + sizes[k]], bufs[k][pad:pad + sizes[k]]), (k, "an owned float was left unwritten")
    return {}


def check_weighting(device, N=6, P=4, d=5):
    """one sample (no overlapping windows), unit weights: a row whose presence is 0 at the start contributes to no sum; a row
    whose presence is 0 at step p0 only is dropped from that step's sums alone; all-zero weights give zeros"""
    case = Case(1, N, P, d, 1, device, seed=3, presence_p=2.0)         # every row present everywhere
    case.weight[:] = 1.0
    case.upload()
    worst = {}
    base = case.run()
    assert_vs_fp64(case, base, worst, "all present")
    assert torch.equal(base["metrics"][0, :, 2].cpu(), torch.full((P,), float(N)))
    t0 = int(case.start[0, 0])
    # (a) row 2 absent at step p0 = 1 only
    p0 = 1
    keep = case.buf.clone()
    case.buf[case._row_index(t0 + 1 + p0, 0, 2)] = 0.0
    case.upload()
    out = case.run()
    assert_vs_fp64(case, out, worst, "absent at one step")
    assert torch.equal(out["pred"], base["pred"]), "the targets entered a prediction"
    m, mb = out["metrics"][0].cpu(), base["metrics"][0].cpu()
    others = [p for p in range(P) if p != p0]
    assert torch.equal(m[others], mb[others]), "another step's sums moved"
    assert float(m[p0, 2]) == N - 1 and float(m[p0, 0]) < float(mb[p0, 0]) and float(m[p0, 1]) < float(mb[p0, 1])
    # (b) row 4 absent at the start
    case.buf = keep.clone()
    case.buf[case._row_index(t0, 0, 4)] = 0.0
    case.upload()
    out = case.run()
    assert_vs_fp64(case, out, worst, "absent at the start")
    assert torch.equal(out["metrics"][0, :, 2].cpu(), torch.full((P,), float(N - 1)))
    # its sums are those of the other rows alone: the same as giving it garbage targets
    case.buf[case._row_index(torch.arange(t0 + 1, t0 + 1 + P), 0, 4) + 1] = 1e30
    case.upload()
    assert torch.equal(case.run()["metrics"], out["metrics"])
    # (c) all weights zero
    case.buf = keep
    case.weight[:] = 0.0
    case.upload()
    out = case.run()
    assert torch.equal(out["metrics"].cpu(), torch.zeros(1, P, 3))
    return worst


def check_repeatable(device, S=5, N=13, P=5, d=5, n_nets=5):
    """three launches, bitwise-equal outputs (an order of summation, not a race, is what this pins)"""
    case = Case(S, N, P, d, n_nets, device, seed=1)
    first = case.run()
    for _ in range(2):
        again = case.run()
        assert torch.equal(again["pred"], first["pred"]) and torch.equal(again["metrics"], first["metrics"])
    return {}


def check_agrees_with_training(device, S=5, N=13, P=5, d=5, n_nets=5):
    """iplan_predict against ops.pdec_forward(keep=None, teacher=None, drop_p=0) on a materialised copy of the same inputs"""
    case = Case(S, N, P, d, n_nets, device, seed=2)
    out = case.run(metrics=False)
    x0, tg = case.gather()
    fwd = ops.pdec_forward(case.arena, x0.reshape(n_nets, S * N, d).contiguous().to(device), case.d_h0,
                           tg.reshape(n_nets, S * N, P, d).contiguous().to(device), torch.ones(n_nets, S, device=device), N)
    _sync(device)
    p64, _ = case.reference(torch.float64)
    p32, _ = case.reference(torch.float32)
    worst = {}
    for n in range(n_nets):
        e32 = _grad_err(p32[n], p64[n])
        err = _grad_err(out["pred"][n], fwd["pred"][n])
        _worse(worst, "vs_training", err)
        assert err <= _bound(e32), (n, err, e32)
    worst["bit_equal"] = float(torch.equal(out["pred"], fwd["pred"]))
    print("iplan_predict vs iplan_pdec_fwd: bit-equal =", bool(worst["bit_equal"]), "worst relative difference", worst["vs_training"])
    return worst


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_args(device, **kw):
    from iplan_amd.config import default_args
    base = dict(use_cuda=torch.device(device).type == "cuda", max_vehicle_num=5, n_agents=2, episode_limit=12, pred_length=3,
                pred_batch_size=6)
    base.update(kw)
    return default_args("highway", **base)


def _gumbel(gen, *shape):
    u = torch.rand(*shape, generator=gen).clamp_min(1e-20)
    return -torch.log((-torch.log(u)).clamp_min(1e-20))


def _loaded_policy(args, tmp_path, seed):
    """a policy whose weights came through load_models from files in the reference's format (one plain state_dict of CPU
    tensors per file, nova/prediction_policy.py:262-268); returns (policy, GAT state dicts, decoder state dicts)"""
    from iplan_amd.nova.prediction_policy import Prediction_policy
    torch.manual_seed(seed)
    src = Prediction_policy(args, _Log())
    gat = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in src.pred_GAT]
    dec = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in src.pred_decoder]
    for i in range(args.n_agents):
        torch.save(gat[i], f"{tmp_path}/pred_GAT_{i}.th")
        torch.save(dec[i], f"{tmp_path}/pred_decoder_{i}.th")
    torch.manual_seed(seed + 100)
    pol = Prediction_policy(args, _Log())
    assert not torch.equal(pol.pred_decoder[0].state_dict()["decoder.out.weight"].cpu(), dec[0]["decoder.out.weight"])
    pol.load_models([str(tmp_path)])
    return pol, gat, dec


def _oracle_pred(gat, dec, hist, att, lat, noise, P, dtype, use_behavior=True):
    """hist [B, N, d], att [B, N, A], lat [B, N, Z], noise [B, N, N-1, 2] of one agent -> [B, N, P, d]"""
    B, N, d = hist.shape
    g, dd = {k: v.to(dtype) for k, v in gat.items()}, {k: v.to(dtype) for k, v in dec.items()}
    obs = torch.cat([hist, lat], -1).to(dtype) if use_behavior else hist.to(dtype)
    hid = O.gat_forward(g, obs, att.reshape(B * N, -1).to(dtype), noise.reshape(-1, 2).to(dtype))
    return O.prediction_decoder_forward(dd, hist.to(dtype).reshape(B, N, 1, d), hid, P)


def check_predict_method(device, tmp_path, E=2):
    """Prediction_policy.predict on a loaded reference-format checkpoint against the oracle chain, numpy in / numpy out and
    device tensors in / device tensor out"""
    from iplan_amd import synth
    args = _e2e_args(device)
    pol, gat, dec = _loaded_policy(args, tmp_path, 11)
    nA, N, P = args.n_agents, args.max_vehicle_num, args.pred_length
    gen = torch.Generator().manual_seed(4)
    hist = synth.make_history(gen, (E, nA), N, args.obs_shape_single, presence_p=0.7)
    att = torch.randn(E, nA, N, args.attention_dim, generator=gen) * 0.1
    lat = torch.softmax(torch.randn(E, nA, N, args.latent_dim, generator=gen), -1)
    noise = _gumbel(gen, nA, E, N, N - 1, 2)
    got = pol.predict(hist.double().numpy(), att.numpy(), lat.numpy(), noise=noise.to(device))
    assert isinstance(got, np.ndarray) and got.shape == (E, nA, N, P, args.obs_shape_single)
    dev_out = pol.predict(hist.to(device), att.to(device), lat.to(device), noise=noise.to(device))
    assert torch.is_tensor(dev_out) and dev_out.device.type == torch.device(device).type
    assert np.array_equal(dev_out.cpu().numpy(), got)
    worst = {}
    for i in range(nA):
        r64 = _oracle_pred(gat[i], dec[i], hist[:, i], att[:, i], lat[:, i], noise[i], P, torch.float64)
        r32 = _oracle_pred(gat[i], dec[i], hist[:, i], att[:, i], lat[:, i], noise[i], P, torch.float32)
        e32, err = _grad_err(r32, r64), _grad_err(torch.as_tensor(got[:, i]), r64)
        print("predict agent", i, "err", err, "e32", e32)
        _worse(worst, "predict", err)
        _worse(worst, "predict_e32", e32)
        assert err <= _bound(e32), (i, err, e32)
    return worst


def _evaluate_loop(gat, dec, f, noise, P, stride, pos, pc, dtype):
    """the plain loop over (episode, start step, agent) evaluate() is defined by; noise [nA, E * n_starts, N, N-1, 2]"""
    hist, att, lat = f["history"][:, :-1], f["attention_latent"][:, :-1], f["behavior_latent"][:, :-1]
    term, filled = f["terminated"][:, :-1], f["filled"][:, :-1]
    E, T, nA, N, d = hist.shape
    sums = torch.zeros(nA, P, 3, dtype=dtype)
    s = 0
    for e in range(E):
        for t in range(0, T - P - 1, stride):
            for i in range(nA):
                if term[e, t:t + P + 1, i, 0].any() or not filled[e, t:t + P + 1, 0].all():
                    continue
                pr = _oracle_pred(gat[i], dec[i], hist[e, t, i][None], att[e, t, i][None], lat[e, t, i][None], noise[i, s][None], P, dtype)[0]
                for p in range(P):
                    tg = hist[e, t + 1 + p, i].to(dtype)
                    w = ((hist[e, t, i, :, pc] != 0) & (tg[:, pc] != 0)).to(dtype)
                    delta = tg - pr[:, p]
                    sums[i, p, 0] += (w * (delta[:, list(pos)] ** 2).sum(-1).sqrt()).sum()
                    sums[i, p, 1] += (w * delta.abs().sum(-1)).sum()
                    sums[i, p, 2] += w.sum()
            s += 1
    return sums


def check_evaluate_method(device, tmp_path, stride, E=2, chunk=5):
    """Prediction_policy.evaluate on a loaded checkpoint against the plain loop: one terminated episode tail, an unfilled step,
    several chunks; deferred == inline; NaN where nothing counts; generators, parameters and optimiser state untouched"""
    from iplan_amd import synth
    args = _e2e_args(device)
    pol, gat, dec = _loaded_policy(args, tmp_path, 13)
    nA, N, P, T = args.n_agents, args.max_vehicle_num, args.pred_length, args.episode_limit
    f = synth.make_episode_fields(args, E, seed=6, terminated_p=0.0)
    gen = torch.Generator().manual_seed(8)
    f["history"] = synth.make_history(gen, (E, T + 1, nA), N, args.obs_shape_single, presence_p=0.7)
    f["terminated"][1, 7:, 0] = 1                                  # agent 0 of episode 1 terminates at step 7
    f["filled"][1, 10:] = 0                                        # and the episode's last steps were never written
    batch = synth.DictBatch(f, E, T + 1).to(device)
    n_starts = len(range(0, T - P - 1, stride))
    assert E * n_starts > chunk
    noise = _gumbel(gen, nA, E * n_starts, N, N - 1, 2)
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), torch=torch.get_rng_state(), numpy=np.random.get_state()[1].copy(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer])
    res = pol.evaluate(batch, stride=stride, noise=noise.to(device), max_samples_per_launch=chunk)
    fin = pol.evaluate(batch, stride=stride, noise=noise.to(device), max_samples_per_launch=chunk, defer=True)
    assert callable(fin)
    res2 = fin()
    assert torch.equal(pol.gat_arena.data, before["gat"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert torch.equal(torch.get_rng_state(), before["torch"]) and np.array_equal(np.random.get_state()[1], before["numpy"])
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"]
    for k in ("displacement", "ade", "fde", "l1", "count"):
        assert isinstance(res[k], np.ndarray) and np.array_equal(res[k], res2[k], equal_nan=True), k
    assert res["displacement"].shape == (nA, P) and res["ade"].shape == (nA,) and res["fde"].shape == (nA,)
    s64 = _evaluate_loop(gat, dec, f, noise, P, stride, (1, 2), 0, torch.float64)
    s32 = _evaluate_loop(gat, dec, f, noise, P, stride, (1, 2), 0, torch.float32)
    worst = {}
    assert np.array_equal(res["count"], s64[..., 2].numpy()), (res["count"], s64[..., 2])
    assert (res["count"] > 0).all() and res["count"][0].max() < res["count"][1].max()       # the terminated agent lost samples
    for key, k in (("displacement", 0), ("l1", 1)):
        for i in range(nA):
            m64, m32 = _means(s64[i])[:, k], _means(s32[i])[:, k]
            e32, err = _grad_err(m32, m64), _grad_err(torch.as_tensor(res[key][i]), m64)
            print("evaluate stride", stride, key, "agent", i, "err", err, "e32", e32)
            _worse(worst, key, err)
            _worse(worst, key + "_e32", e32)
            assert err <= _bound(e32), (key, i, err, e32)
    ade64 = s64[..., 0].sum(1) / s64[..., 2].sum(1)
    ade32 = (s32[..., 0].sum(1) / s32[..., 2].sum(1)).double()
    e32, err = _grad_err(ade32, ade64), _grad_err(torch.as_tensor(res["ade"]), ade64)
    _worse(worst, "ade", err)
    assert err <= _bound(e32), ("ade", err, e32)
    assert np.array_equal(res["fde"], res["displacement"][:, -1])
    # chunking only changes the order the sums are added in
    one = pol.evaluate(batch, stride=stride, noise=noise.to(device), max_samples_per_launch=10 ** 6)
    assert np.array_equal(one["count"], res["count"])
    assert _grad_err(torch.as_tensor(one["displacement"]), torch.as_tensor(res["displacement"])) < 1e-6
    # nothing counts: NaN, no exception
    f2 = dict(f)
    f2["terminated"] = torch.ones_like(f["terminated"])
    none = pol.evaluate(synth.DictBatch(f2, E, T + 1).to(device), stride=stride, noise=noise.to(device), max_samples_per_launch=chunk)
    assert (none["count"] == 0).all()
    for k in ("displacement", "l1", "ade", "fde"):
        assert np.isnan(none[k]).all(), k
    # without injected noise it draws its own and still returns finite numbers
    own = pol.evaluate(batch, stride=stride, max_samples_per_launch=chunk)
    assert np.isfinite(own["ade"]).all() and np.array_equal(own["count"], res["count"])
    return worst


def check_learn_unaffected_by_evaluate(device, E=2):
    """learn() with injected sel / noise / keep gives the same loss and the same parameters whether or not an evaluate() ran
    before it"""
    from iplan_amd import synth
    from iplan_amd.nova.prediction_policy import Prediction_policy
    args = _e2e_args(device)
    nA, N, P, S = args.n_agents, args.max_vehicle_num, args.pred_length, args.pred_batch_size
    batch = synth.make_batch(args, E, seed=9, terminated_p=0.1, device=device)
    gen = torch.Generator().manual_seed(21)
    avail = args.episode_limit - P - 1
    sel = torch.stack([torch.randperm(E * avail, generator=gen)[:S] for _ in range(nA)]).numpy()
    noise = _gumbel(gen, nA, S, N, N - 1, 2).to(device)
    keep = (torch.rand(nA, P, S * N, args.attention_dim, generator=gen) < 1.0 - args.decoder_dropout).float().to(device)
    results = []
    for with_eval in (False, True):
        torch.manual_seed(31)
        np.random.seed(32)
        pol = Prediction_policy(args, _Log())
        if with_eval:
            ev = pol.evaluate(batch, stride=3, max_samples_per_launch=4, noise=_gumbel(gen, nA, E * len(range(0, avail, 3)), N, N - 1, 2).to(device))
            assert np.isfinite(ev["ade"]).all()
        losses = pol.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), pol.gat_arena.data.clone(), pol.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}
