"""TEST INFRASTRUCTURE: the three PPO learning kernels alone (csrc/ppo.hip: iplan_ppo_prepare, iplan_ppo_adv_norm, iplan_ppo_loss), each
in every launch form, on whatever library is active -- the host emulator in tests/test_emu_ppo_learn.py, the gfx950 build in
tests/test_gpu_ppo_learn.py.  The descriptors are filled directly and launched with ``lib.call``.

Ground truth: the unchanged oracle in fp64 torch -- oracle.gae_returns, normalise_advantages, ppo_losses -- and, for the row gradients,
fp64 autograd of it: g_logp = d policy_loss / d logp, g_values = d (value_loss_coef x value_loss) / d values, value_loss_coef = 0.5.
The same oracle runs in fp32 beside it.  Rule: error = max|got - ref64| / max(1, max|ref64|) per agent and
tensor, for the two gradient tensors relative to the tensor's own scale (oracle_checks._grad_err); bound = max(1e-5, E32_FACTOR x e32),
e32 the fp32 oracle's error by the same measure.  A tensor whose fp64 value is identically zero must be exactly zero, and so must every
ROW gradient that fp64 autograd gives as exactly zero: a zero there is a branch (a dead row's weight, the clipped side of a min / max,
the flat side of the one-sided Huber loss), and the inputs keep every row MARGIN away from every branch point, so fp32 takes the same
one.  mask, value_preds and stats[4] are exact.

Inputs of the loss (make_rows): no row within MARGIN, measured in fp64, of |ratio - 1| = clip, of |values - value_preds| = clip, of the
one-sided Huber jump e = -delta for either residual, or -- where |dv| > clip -- of h1 = h2 (Huber and MSE form both, so one draw serves
every ``flags``); asserted on the reference, together with: every branch occurs among the live rows of every agent (SMALL shapes
exempt).  EDGE rows sit exactly ON an edge where fp32 and fp64 decide alike bit for bit.  The seeds (SEEDS) were found on the CPU from
the oracle alone (pick_seed).  The checks never touch ``L.use_library_for_tests``; each returns the worst errors it measured."""
import ctypes as C
import functools

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.ac_backward_checks import _sentinel
from tests.oracle_checks import E32_FACTOR, _grad_err
from tests.ppo_eval_checks import CLIP, HUBER, MARGIN, _bits, _einval, _sync, _worse, flag_kwargs

TOL = 1e-5
VCOEF = 0.5                                                        # not 1: a dropped factor shows
GAMMA, LAM = float(np.float32(0.99)), float(np.float32(0.95))      # (the fp32 values the kernel gets)
FENCE = 64
ALL_FLAGS = L.PPO_MSE | L.PPO_NO_VCLIP | L.PPO_VALUE_MEAN | L.PPO_POLICY_MEAN

# ---- iplan_ppo_prepare: (bs, T) -- n = 2 (the smallest accepted) both ways; n at the wave and workgroup edges; the thread-strided
# episode loop past 1024 episodes, alone and with T = 3 (3075 rows: the largest launch); a long recursion
PREP_SHAPES = [(2, 1), (1, 2), (3, 7), (63, 1), (64, 1), (65, 1), (1023, 1), (1024, 1), (1025, 1), (1025, 3), (7, 147)]
LAYOUTS = ("batch", "agent")
# ---- iplan_ppo_adv_norm: rows of rank 0 and rank 1
NORM_PAIRS = [(1, 63), (63, 65), (65, 1024), (1024, 1025), (1025, 1)]
NORM_ONE_RANK = [(2, 1), (3, 7), (1024, 1), (1025, 3), (7, 147)]
# ---- iplan_ppo_loss
LOSS_ROWS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
SMALL = (1, 2, 5)                                                  # too few rows for every branch (and for the EDGE rows)
# (n_agents, rows, live, flags)
LOSS_CASES = ([(nA, r, "drawn", 0) for r in LOSS_ROWS for nA in (1, 3)] + [(nA, r, "all", 0) for r in (65, 1025) for nA in (1, 3)]
              + [(nA, r, "drawn", f) for f in (L.PPO_MSE, L.PPO_NO_VCLIP, L.PPO_VALUE_MEAN, L.PPO_POLICY_MEAN) for r in (65, 1025) for nA in (1, 3)]
              + [(nA, 65, "drawn", ALL_FLAGS) for nA in (1, 3)])
LOSS_IDS = [f"nA{a}_rows{r}_{lv}_flags{f}" for a, r, lv, f in LOSS_CASES]
# (rows, P): per = ceil(rows / P) leaves the last range short at (65,2)/(1025,2)/(1025,3), one row per range at (65,65), and trailing
# ranges EMPTY at (5,4) (per 2: range 3), (65,64) (per 2: ranges 33 ..), (2049,64) (per 33: range 63) and (1025,1024) (per 2: 513 ..)
PART_CASES = [(5, 4), (65, 2), (65, 64), (65, 65), (1025, 2), (1025, 3), (2049, 64), (1025, 1024)]
# rows 3 .. 7 of every agent where rows >= 63: exactly ON an edge (see make_rows)
EDGE = dict(same_logp=3, zero_adv=4, dv_plus=5, dv_minus=6, flat=7)
# seed of every (n_agents, rows, live): the first at which the draw meets the conditions (pick_seed; CPU, oracle only)
SEEDS = {(nA, r, "drawn"): 0 for nA in (1, 3) for r in LOSS_ROWS + (5,)}
SEEDS.update({(nA, r, "all"): 0 for nA in (1, 3) for r in (65, 1025)})
SEEDS.update({(3, 63, "drawn"): 1, (1, 65, "drawn"): 1})           # (seed 0 there misses a branch)


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def _rule(got, r64, r32, worst, key, what, own_scale=False):
    """got / r64 / r32 [nA, ...]: the rule per agent; every figure is printed before it is asserted"""
    for i in range(r64.shape[0]):
        g, a, b = got[i].detach().cpu().double(), r64[i].double(), r32[i].double()
        assert torch.isfinite(g).all(), (what, key, i, "not finite")
        if not a.any():
            assert not g.any(), (what, key, i, "fp64 is identically zero, the kernel's is not")
            continue
        if own_scale:
            err, e32 = _grad_err(g, a), _grad_err(b, a)
            assert not g[a == 0].any(), (what, key, i, "a row gradient that is exactly zero in fp64 is not zero")
        else:
            scale = max(1.0, a.abs().max().item())
            err, e32 = (g - a).abs().max().item() / scale, (b - a).abs().max().item() / scale
        print(what, key, "agent", i, "err", err, "e32", e32, "bound", _bound(e32))
        _worse(worst, key, err)
        _worse(worst, key + "_e32", e32)
        assert err <= _bound(e32), (what, key, i, err, e32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu())), (what, "bits differ")


def _nan(*shape, device):
    return torch.full(shape, float("nan"), device=device)


def _fenced(shape, device):
    """a [shape] view FENCE floats into a sentinel-filled buffer -> (the pattern on the host, the buffer, the view)"""
    n = int(np.prod(shape))
    sent = _sentinel(n + 2 * FENCE, "cpu")
    buf = sent.clone().to(device)
    return sent, buf, buf[FENCE:FENCE + n].view(shape)


def _fence_intact(sent, buf, n, what):
    host = buf.cpu()
    assert torch.equal(_bits(host[:FENCE]), _bits(sent[:FENCE])) and torch.equal(_bits(host[FENCE + n:]), _bits(sent[FENCE + n:])), (what, "written outside its extent")


# ================================================================================================ iplan_ppo_prepare
@functools.lru_cache(maxsize=None)
def make_episodes(nA, bs, T, seed=0):
    """fp32 / uint8 host tensors in the learner's batch layout, never modified: reward, terminated [bs, T + 1, nA, 1], values
    [nA, bs, T + 1].  terminated ~ Bernoulli(0.2); forced where there is room: episode 0 dead from t = 0, episode 1 terminated only at
    t = T (that touches the bootstrap alone), episode 2 fully live; with three agents the last one is dead but for two rows"""
    gen = torch.Generator().manual_seed(9000 + 131 * bs + 17 * T + nA + 1000 * seed)
    reward = torch.randn(bs, T + 1, nA, 1, generator=gen)
    term = (torch.rand(bs, T + 1, nA, 1, generator=gen) < 0.2).to(torch.uint8)
    v_all = torch.randn(nA, bs, T + 1, generator=gen)
    if bs >= 3:
        term[0] = 1
        term[1] = 0
        term[1, T] = 1
        term[2] = 0
    elif bs == 2:
        term[0] = 0
        term[0, T] = 1
        term[1] = 0
    if nA == 3 and bs * T > 2:
        term[:, :, 2] = 1
        term[bs - 1, 0, 2] = 0
        term[bs // 2, T - 1, 2] = 0
        assert (1 - term[:, :T, 2].float()).sum() == 2
    return dict(dims=(nA, bs, T), reward=reward, terminated=term, values=v_all)


@functools.lru_cache(maxsize=None)
def prepare_reference(nA, bs, T, no_gae, dt):
    """-> returns, adv_raw, adv_norm, mask, value_preds [nA, bs T] in ``dt`` (the oracle, unchanged)"""
    ep = make_episodes(nA, bs, T)
    out = {k: [] for k in ("returns", "adv_raw", "adv_norm", "mask", "value_preds")}
    for i in range(nA):
        rw = ep["reward"][:, :T, i].to(dt)
        v = ep["values"][i].to(dt).unsqueeze(-1)
        m = 1.0 - ep["terminated"][:, :, i].to(dt)
        rets = O.gae_returns(rw, v, m, GAMMA, LAM, not no_gae)
        raw = (rets - v[:, :-1]).clone()
        raw[m[:, :-1] == 0.0] = 0.0
        for k, t in (("returns", rets), ("adv_raw", raw), ("adv_norm", O.normalise_advantages(rets, v[:, :-1], m[:, :-1])), ("mask", m[:, :-1]),
                     ("value_preds", v[:, :-1])):
            out[k].append(t.reshape(-1))
    return {k: torch.stack(v) for k, v in out.items()}


def run_prepare(device, ep, layout, skip_norm, no_gae, outs=None):
    """one iplan_ppo_prepare launch; outputs pre-filled with NaN unless given -> dict of [nA, bs T] device tensors"""
    nA, bs, T = ep["dims"]
    if layout == "batch":                                     # [bs, T + 1, nA, 1], the strides train() passes
        rw, tm = ep["reward"].to(device), ep["terminated"].to(device)
        rs, ts = (rw.stride(2), rw.stride(0), rw.stride(1)), (tm.stride(2), tm.stride(0), tm.stride(1))
    else:                                                     # contiguous per agent: [nA, bs, T + 1]
        rw, tm = (ep[k][..., 0].permute(2, 0, 1).contiguous().to(device) for k in ("reward", "terminated"))
        rs, ts = tuple(rw.stride()), tuple(tm.stride())
    va = ep["values"].to(device)
    pp = L.PpoPrepareArgs()
    pp.n_agents, pp.bs, pp.T = nA, bs, T
    pp.reward, pp.rw_s_net, pp.rw_s_ep, pp.rw_s_t = rw.data_ptr(), *rs
    pp.terminated, pp.tm_s_net, pp.tm_s_ep, pp.tm_s_t = tm.data_ptr(), *ts
    pp.values, pp.gamma, pp.lam = va.data_ptr(), GAMMA, LAM
    names = ("returns", "adv", "mask", "value_preds")
    outs = outs or {k: _nan(nA, bs * T, device=device) for k in names}
    pp.returns, pp.adv, pp.mask, pp.value_preds = (outs[k].data_ptr() for k in names)
    pp.skip_norm, pp.no_gae = skip_norm, no_gae
    ops._lib(None).call("iplan_ppo_prepare", pp, L.current_stream(device))
    _sync(device)
    return outs


def check_prepare(device, nA, bs, T):
    """1: skip_norm x no_gae x layout against fp64: returns and adv by the rule, mask and value_preds bitwise, raw adv exactly 0 on dead
    rows, everything but adv the same bits with and without the normalisation, and both layouts the same bits"""
    worst = {}
    ep = make_episodes(nA, bs, T)
    for no_gae in (0, 1):
        r64, r32 = prepare_reference(nA, bs, T, no_gae, torch.float64), prepare_reference(nA, bs, T, no_gae, torch.float32)
        first = {}
        for layout in LAYOUTS:
            got = {s: run_prepare(device, ep, layout, s, no_gae) for s in (0, 1)}
            what = ("prepare", nA, bs, T, layout, "no_gae" if no_gae else "gae")
            for s in (0, 1):
                _same(got[s]["mask"], r32["mask"], what + ("mask",))
                _same(got[s]["value_preds"], r32["value_preds"], what + ("value_preds",))
                _rule(got[s]["returns"], r64["returns"], r32["returns"], worst, "returns", what)
            _rule(got[1]["adv"], r64["adv_raw"], r32["adv_raw"], worst, "adv_raw", what)
            _rule(got[0]["adv"], r64["adv_norm"], r32["adv_norm"], worst, "adv_norm", what)
            assert not got[1]["adv"].cpu()[r64["mask"] == 0].any(), (what, "raw advantage of a dead row is not exactly 0")
            for k in ("returns", "mask", "value_preds"):
                _same(got[0][k], got[1][k], what + (k, "skip_norm changed it"))
            for s in (0, 1):
                for k, v in got[s].items():
                    _same(v, first.setdefault((s, k), v), what + (k, "the layout changed it"))
    return worst


# ================================================================================================ iplan_ppo_adv_norm
def run_adv_norm(device, adv, n, count, phase, asum, asq):
    an = L.AdvNormArgs()
    an.n_agents, an.n, an.row_stride = adv.shape[0], n, adv.stride(0)
    an.adv, an.sum, an.sqdev = adv.data_ptr(), asum.data_ptr(), asq.data_ptr()
    an.count, an.phase = float(count), phase
    ops._lib(None).call("iplan_ppo_adv_norm", an, L.current_stream(device))
    _sync(device)


def check_adv_norm_two_ranks(device, nA, n0, n1):
    """2a: two ranks played on one device -- phase 0 on both, the [nA] sums added (all an all-reduce does), phase 1 on both, added,
    phase 2 on both; the concatenation against fp64 normalise_advantages over all rows; nothing past ``n`` is touched"""
    gen = torch.Generator().manual_seed(77 + 13 * n0 + n1 + nA)
    raw = torch.randn(nA, n0 + n1, generator=gen) * (torch.rand(nA, n0 + n1, generator=gen) < 0.8).float()
    r64, r32 = (torch.stack([O.normalise_advantages(x, torch.zeros_like(x), torch.ones_like(x)) for x in raw.to(dt)]) for dt in (torch.float64, torch.float32))
    ranks = []
    for lo, n in ((0, n0), (n0, n1)):
        sent = _sentinel(nA * (n + 5), "cpu").view(nA, n + 5)
        buf = sent.clone()
        buf[:, :n] = raw[:, lo:lo + n]
        ranks.append(dict(n=n, sent=sent, adv=buf.to(device), sum=_nan(nA, device=device), sq=_nan(nA, device=device)))
    count = n0 + n1
    for phase, red in ((0, "sum"), (1, "sq"), (2, None)):
        for r in ranks:
            run_adv_norm(device, r["adv"], r["n"], count, phase, r["sum"], r["sq"])
        if red is not None:
            total = ranks[0][red] + ranks[1][red]
            for r in ranks:
                r[red].copy_(total)
    got = torch.cat([r["adv"][:, :r["n"]] for r in ranks], dim=1)
    worst = {}
    _rule(got, r64, r32, worst, "adv_norm", ("adv_norm", nA, n0, n1))
    for r in ranks:
        assert torch.equal(_bits(r["adv"][:, r["n"]:].cpu()), _bits(r["sent"][:, r["n"]:])), ("adv_norm", n0, n1, "wrote past n")
    return worst


def check_adv_norm_one_rank(device, bs, T, nA=3):
    """2b: one rank, count = n, on the raw advantages iplan_ppo_prepare(skip_norm = 1) leaves: the bits of skip_norm = 0 (the header's
    "reproduces iplan_ppo_prepare's own normalisation")"""
    ep = make_episodes(nA, bs, T)
    raw, normed = run_prepare(device, ep, "batch", 1, 0)["adv"], run_prepare(device, ep, "batch", 0, 0)["adv"]
    adv = raw.clone()
    asum, asq = _nan(nA, device=device), _nan(nA, device=device)
    for phase in (0, 1, 2):
        run_adv_norm(device, adv, bs * T, bs * T, phase, asum, asq)
    _same(adv, normed, ("adv_norm with one rank against prepare's own normalisation", bs, T))
    return {}


# ================================================================================================ iplan_ppo_loss: inputs
def _huber(e):
    return O.huber_loss(e, HUBER)


def _mse(e):
    return e ** 2 / 2


def _quantities(inp, rows):
    """the fp64 quantities the branches hang on, [nA, rows]"""
    d = lambda k: inp[k][:, :rows].double()  # noqa: E731
    ratio = torch.exp(d("logp") - d("old_logp"))
    dv = d("values") - d("value_preds")
    vc = d("value_preds") + dv.clamp(-CLIP, CLIP)
    return ratio, dv, d("returns") - d("values"), d("returns") - vc


def _near(inp, rows, margin):
    ratio, dv, e1, e2 = _quantities(inp, rows)
    near = ((ratio - 1).abs() - CLIP).abs() < margin
    near |= (dv.abs() - CLIP).abs() < margin
    near |= ((e1 + HUBER).abs() < margin) | ((e2 + HUBER).abs() < margin)
    for loss in (_huber, _mse):
        near |= (dv.abs() > CLIP) & ((loss(e1) - loss(e2)).abs() < margin)
    return near


def _branches(inp, rows):
    """per agent over the live rows: name -> whether the branch occurs"""
    ratio, dv, e1, e2 = _quantities(inp, rows)
    live, adv = inp["mask"][:, :rows] != 0, inp["adv"][:, :rows]
    out = dv.abs() > CLIP
    sets = dict(ratio_high_adv_pos=(ratio > 1 + CLIP) & (adv > 0), ratio_high_adv_neg=(ratio > 1 + CLIP) & (adv < 0),
                ratio_low_adv_pos=(ratio < 1 - CLIP) & (adv > 0), ratio_low_adv_neg=(ratio < 1 - CLIP) & (adv < 0),
                ratio_inside_adv_pos=((ratio - 1).abs() < CLIP) & (adv > 0), ratio_inside_adv_neg=((ratio - 1).abs() < CLIP) & (adv < 0),
                value_clipped=out, value_inside=~out, huber_quadratic=e1.abs() <= HUBER, huber_linear=e1 > HUBER, huber_flat=e1 < -HUBER,
                huber_h1_above=out & (_huber(e1) > _huber(e2)), huber_h2_above=out & (_huber(e2) > _huber(e1)),
                mse_h1_above=out & (_mse(e1) > _mse(e2)), mse_h2_above=out & (_mse(e2) > _mse(e1)))
    return {k: (v & live).any(dim=1) for k, v in sets.items()}


def build_rows(nA, rows, live, seed):
    """fp32 host tensors of one loss case at ``seed``: logp / entropy / values [nA, rows], old_logp / adv / value_preds / returns / mask
    [nA, rows + 3].  Raises AssertionError when the draw misses a condition (pick_seed then tries the next seed)"""
    stride = rows + 3
    gen = torch.Generator().manual_seed(100000 * seed + 31 * rows + nA + (7 if live == "all" else 0))
    rnd = lambda: torch.randn(nA, stride, generator=gen)  # noqa: E731
    logp, delta, values, dv, res = -1.2 + 0.5 * rnd(), 0.2 * rnd(), rnd(), 0.25 * rnd(), rnd()
    adv = rnd()
    entropy = 0.2 + 1.4 * torch.rand(nA, stride, generator=gen)
    mask = torch.ones(nA, stride) if live == "all" else (torch.rand(nA, stride, generator=gen) < 0.7).float()
    for i in range(nA):
        if mask[i, :rows].sum() < min(2, rows):
            mask[i, :2] = 1
    for _ in range(200):                                      # redraw the rows next to a branch point
        inp = dict(logp=logp, old_logp=logp - delta, values=values, value_preds=values - dv, returns=values + res)
        bad = _near(inp, stride, 2 * MARGIN)
        if not bad.any():
            break
        delta, dv, res = torch.where(bad, 0.2 * rnd(), delta), torch.where(bad, 0.25 * rnd(), dv), torch.where(bad, rnd(), res)
    else:
        raise AssertionError(("no admissible draw", nA, rows, live, seed))
    old, vp, ret = logp - delta, values - dv, values + res
    if rows not in SMALL:
        e = EDGE
        mask[:, min(e.values()):max(e.values()) + 1] = 1
        old[:, e["same_logp"]] = logp[:, e["same_logp"]]      # ratio exactly 1: a tie inside the clip, gradient = -w adv
        adv[:, e["zero_adv"]] = 0.0                           # both surrogates 0 with the ratio outside the clip: gradient exactly 0
        old[:, e["zero_adv"]] = logp[:, e["zero_adv"]] - 0.5
        for k, sign in (("dv_plus", 1.0), ("dv_minus", -1.0)):   # dv exactly on the inclusive clip edge: clipped value == value, h1 == h2
            vp[:, e[k]] = 0.0
            values[:, e[k]] = sign * CLIP
            ret[:, e[k]] = values[:, e[k]] + 0.3
        values[:, e["flat"]], vp[:, e["flat"]], ret[:, e["flat"]] = 0.5, 0.4, -1.5   # both residuals below -delta: Huber loss and gradient 0
    inp = dict(logp=logp[:, :rows].contiguous(), entropy=entropy[:, :rows].contiguous(), values=values[:, :rows].contiguous(), old_logp=old, adv=adv,
               value_preds=vp, returns=ret, mask=mask)
    # ---- the conditions, on the fp64 reference
    random_rows = torch.ones(rows, dtype=torch.bool)
    if rows not in SMALL:
        random_rows[list(EDGE.values())] = False
        ratio, dvv, e1, e2 = _quantities(inp, rows)
        e = EDGE
        assert (ratio[:, e["same_logp"]] == 1).all() and (torch.exp(inp["logp"] - old[:, :rows])[:, e["same_logp"]] == 1).all()
        assert ((ratio[:, e["zero_adv"]] - 1).abs() > CLIP + 0.1).all()
        assert (dvv[:, e["dv_plus"]] == CLIP).all() and (dvv[:, e["dv_minus"]] == -CLIP).all()
        assert ((inp["values"] - vp[:, :rows])[:, e["dv_plus"]] == np.float32(CLIP)).all() and (e1[:, [e["dv_plus"], e["dv_minus"]]] == e2[:, [e["dv_plus"], e["dv_minus"]]]).all()
        assert (e1[:, e["flat"]] < -HUBER - 0.1).all() and (e2[:, e["flat"]] < -HUBER - 0.1).all() and (dvv[:, e["flat"]].abs() < CLIP - 0.05).all()
        missing = [(k, v.tolist()) for k, v in _branches(inp, rows).items() if not v.all()]
        assert not missing, ("a branch does not occur", nA, rows, live, seed, missing)
    assert not _near(inp, rows, MARGIN)[:, random_rows].any()
    assert ((mask[:, :rows] != 0).sum(1) >= min(2, rows)).all()
    return inp


def pick_seed(nA, rows, live, tries=200):
    """the first seed at which build_rows' conditions hold (CPU, oracle only)"""
    for seed in range(tries):
        try:
            build_rows(nA, rows, live, seed)
            return seed
        except AssertionError:
            continue
    raise AssertionError(("no seed found", nA, rows, live))


@functools.lru_cache(maxsize=None)
def make_rows(nA, rows, live="drawn"):
    """the committed case: never modified"""
    return build_rows(nA, rows, live, SEEDS[(nA, rows, live)])


# ================================================================================================ iplan_ppo_loss: reference and launch
def reference_rows(inp, rows, flags, dt):
    """oracle.ppo_losses and its autograd in ``dt`` over the first ``rows`` rows of every agent -> g_logp, g_values [nA, rows], stats [nA, 5]"""
    out = dict(g_logp=[], g_values=[], stats=[])
    for i in range(inp["logp"].shape[0]):
        c = lambda k: inp[k][i, :rows].to(dt).reshape(-1, 1)  # noqa: E731
        logp, values = c("logp").requires_grad_(), c("values").requires_grad_()
        ent, m = c("entropy").mean(), c("mask")
        _, pol, critic_objective, vloss, ratio = O.ppo_losses(logp, ent, values, c("old_logp"), c("adv"), c("value_preds"), c("returns"), m,
                                                              CLIP, HUBER, 0.01, VCOEF, **flag_kwargs(flags))
        out["g_logp"].append(torch.autograd.grad(pol, logp)[0][:, 0])
        out["g_values"].append(torch.autograd.grad(critic_objective, values)[0][:, 0])
        out["stats"].append(torch.stack([pol, vloss, ratio.mean(), ent, m.sum()]).detach())
    return {k: torch.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def loss_reference(nA, rows, live, flags, dt):
    return reference_rows(make_rows(nA, rows, live), rows, flags, dt)


def _mask_sum(inp, rows, device):
    return inp["mask"][:, :rows].sum(dim=1).contiguous().to(device)           # (0 / 1 entries: exact in any order)


def run_loss(device, inp, rows, flags, n_parts=0, mask_sum=None, row_count=0.0, outs=None):
    """one iplan_ppo_loss launch with value_loss_coef = VCOEF; g_logp / g_values [nA, rows] and stats [nA, max(1, n_parts), 8] pre-filled
    with NaN unless given -> dict of device tensors"""
    d = {k: v.to(device).contiguous() for k, v in inp.items()}
    nA, stride = d["old_logp"].shape
    assert d["logp"].shape == (nA, rows)
    pl = L.PpoLossArgs()
    pl.n_agents, pl.rows, pl.row_stride = nA, rows, stride
    pl.logp, pl.entropy, pl.values = d["logp"].data_ptr(), d["entropy"].data_ptr(), d["values"].data_ptr()
    pl.old_logp, pl.adv, pl.value_preds = d["old_logp"].data_ptr(), d["adv"].data_ptr(), d["value_preds"].data_ptr()
    pl.returns, pl.mask = d["returns"].data_ptr(), d["mask"].data_ptr()
    pl.clip, pl.huber_delta, pl.value_loss_coef, pl.flags = CLIP, HUBER, VCOEF, flags
    outs = outs or dict(g_logp=_nan(nA, rows, device=device), g_values=_nan(nA, rows, device=device), stats=_nan(nA, max(1, n_parts), 8, device=device))
    pl.g_logp, pl.g_values, pl.stats = outs["g_logp"].data_ptr(), outs["g_values"].data_ptr(), outs["stats"].data_ptr()
    pl.n_parts, pl.row_count = n_parts, row_count
    if mask_sum is not None:
        pl.mask_sum = mask_sum.data_ptr()
    ops._lib(None).call("iplan_ppo_loss", pl, L.current_stream(device))
    _sync(device)
    return outs


def _add_shares(stats):
    """[nA, P, 8] -> [nA, 4]: the P shares added in part order in fp32, as the caller adds them"""
    st = stats.cpu()
    total = st[:, 0, :4].clone()
    for p in range(1, st.shape[1]):
        total = total + st[:, p, :4]
    return total


def _assert_loss(got, r64, r32, worst, what, stats=None):
    _rule(got["g_logp"], r64["g_logp"], r32["g_logp"], worst, "g_logp", what, own_scale=True)
    _rule(got["g_values"], r64["g_values"], r32["g_values"], worst, "g_values", what, own_scale=True)
    stats = got["stats"][:, 0].cpu() if stats is None else stats
    for k, name in enumerate(("policy_loss", "value_loss", "ratio_mean", "dist_entropy")):
        _rule(stats[:, k:k + 1], r64["stats"][:, k:k + 1], r32["stats"][:, k:k + 1], worst, name, what)


def _assert_edges(got, inp, rows, flags, what):
    """the rows built on an edge: exact zeros where the gradient is zero; at ratio == 1 the gradient is -w adv, one rounded division
    and one rounded product away from it: 2 x 2^-24 relative and a second-order term, held to 3 x 2^-24"""
    if rows in SMALL:
        return
    g_lp, g_v = got["g_logp"].cpu(), got["g_values"].cpu()
    e = EDGE
    assert not g_lp[:, e["zero_adv"]].any(), (what, "adv == 0 outside the clip: g_logp is not exactly 0")
    if not flags & L.PPO_MSE:
        assert not g_v[:, e["flat"]].any(), (what, "both residuals below -delta: g_values is not exactly 0")
    w = (1.0 / rows) if flags & L.PPO_POLICY_MEAN else 1.0 / inp["mask"][:, :rows].double().sum(1)
    ref = -w * inp["adv"][:, e["same_logp"]].double()
    assert ((g_lp[:, e["same_logp"]].double() - ref).abs() <= 3 * 2.0 ** -24 * ref.abs()).all(), (what, "ratio == 1: g_logp is not -w adv", g_lp[:, e["same_logp"]], ref)


def check_loss(device, nA, rows, live, flags):
    """3 (forms A and B): n_parts = 0 without and with the caller's mask_sum / row_count, against fp64; stats[4] exact; 5 .. 7 untouched"""
    worst = {}
    inp = make_rows(nA, rows, live)
    r64, r32 = loss_reference(nA, rows, live, flags, torch.float64), loss_reference(nA, rows, live, flags, torch.float32)
    forms = dict(A=run_loss(device, inp, rows, flags), B=run_loss(device, inp, rows, flags, mask_sum=_mask_sum(inp, rows, device), row_count=float(rows)))
    for form, got in forms.items():
        what = ("loss", form, nA, rows, live, flags)
        _assert_loss(got, r64, r32, worst, what)
        _assert_edges(got, inp, rows, flags, what)
        _same(got["stats"][:, 0, 4], r32["stats"][:, 4], what + ("stats[4] is not sum(mask)",))
        assert torch.isnan(got["stats"][:, 0, 5:]).all(), (what, "stats[5..7] were written")
    return worst


def check_loss_parts(device, nA, rows, P, flags=0):
    """3 (form C): n_parts = P > 1 against fp64 and against form B on the same mask_sum"""
    worst = {}
    inp = make_rows(nA, rows, "drawn")
    r64, r32 = loss_reference(nA, rows, "drawn", flags, torch.float64), loss_reference(nA, rows, "drawn", flags, torch.float32)
    msum = _mask_sum(inp, rows, device)
    one = run_loss(device, inp, rows, flags, mask_sum=msum, row_count=float(rows))
    got = run_loss(device, inp, rows, flags, n_parts=P, mask_sum=msum, row_count=float(rows))
    what = ("loss", "C", nA, rows, P, flags)
    st = got["stats"].cpu()
    assert st.shape == (nA, P, 8) and torch.isfinite(st[..., :5]).all(), (what, "a share was left unwritten or is not finite")
    assert torch.isnan(st[..., 5:]).all(), (what, "stats[5..7] were written")
    per = -(-rows // P)
    empty = [p for p in range(P) if p * per >= rows]
    assert bool(empty) == ((rows, P) in ((5, 4), (65, 64), (2049, 64), (1025, 1024))), (what, empty)
    assert not st[:, empty, :5].any(), (what, "an empty range's share is not exactly zero")
    _same(st[:, 0, 4], r32["stats"][:, 4], what + ("stats[0][4] is not the mask sum",))
    assert not st[:, 1:, 4].any(), (what, "stats[p > 0][4] is not zero")
    _assert_loss(got, r64, r32, worst, what, stats=_add_shares(st))
    _assert_edges(got, inp, rows, flags, what)
    for k in ("g_logp", "g_values"):
        _same(got[k], one[k], what + (k, "differs from one workgroup's on the same mask_sum"))
    return worst


def check_loss_two_ranks(device, nA=3, rows=1025, cut=400):
    """3 (data-parallel form): one case's rows cut into two ranks, each launched with the GLOBAL mask_sum and row_count; the ranks'
    stats[0] and stats[1] added, and each rank's row gradients, against the fp64 loss over all rows"""
    worst = {}
    inp = make_rows(nA, rows, "drawn")
    msum = _mask_sum(inp, rows, device)
    assert (inp["mask"][:, :cut].sum(1) != inp["mask"][:, :rows].sum(1)).all()
    for flags in (0, L.PPO_VALUE_MEAN | L.PPO_POLICY_MEAN):
        r64, r32 = loss_reference(nA, rows, "drawn", flags, torch.float64), loss_reference(nA, rows, "drawn", flags, torch.float32)
        total = None
        for rank, (lo, hi) in enumerate(((0, cut), (cut, rows))):
            n = hi - lo
            part = {k: v[:, lo:hi].contiguous() for k, v in inp.items() if k in ("logp", "entropy", "values")}
            for k in ("old_logp", "adv", "value_preds", "returns", "mask"):
                part[k] = torch.cat([inp[k][:, lo:hi], torch.full((nA, 3), float("nan"))], dim=1)
            got = run_loss(device, part, n, flags, n_parts=2 * rank, mask_sum=msum, row_count=float(rows))
            what = ("loss", "two ranks", rank, flags)
            for k in ("g_logp", "g_values"):
                _rule(got[k], r64[k][:, lo:hi], r32[k][:, lo:hi], worst, k, what, own_scale=True)
            share = _add_shares(got["stats"])[:, :2]
            total = share if total is None else total + share
        for k, name in enumerate(("policy_loss", "value_loss")):
            _rule(total[:, k:k + 1], r64["stats"][:, k:k + 1], r32["stats"][:, k:k + 1], worst, name, ("loss", "two ranks", flags))
    return worst


# ================================================================================================ ownership and repeatability
def check_loss_ownership(device, n_parts, nA=3, rows=65):
    """4: outputs inside sentinel-filled buffers -- only [nA, rows] and stats[.., 0..4] change; NaN in the inputs' [rows, row_stride)
    changes no bit; a second launch gives the same bits"""
    inp = make_rows(nA, rows, "drawn")
    P = max(1, n_parts)
    msum = _mask_sum(inp, rows, device) if n_parts else None
    plain = run_loss(device, inp, rows, 0, n_parts=n_parts, mask_sum=msum)
    for k, v in run_loss(device, inp, rows, 0, n_parts=n_parts, mask_sum=msum).items():
        assert torch.equal(_bits(v.cpu()), _bits(plain[k].cpu())), (k, "a second launch differs")                 # (NaN pre-fill included)
    fenced = {k: _fenced(s, device) for k, s in (("g_logp", (nA, rows)), ("g_values", (nA, rows)), ("stats", (nA, P, 8)))}
    run_loss(device, inp, rows, 0, n_parts=n_parts, mask_sum=msum, outs={k: v[2] for k, v in fenced.items()})
    for k, (sent, buf, view) in fenced.items():
        _fence_intact(sent, buf, view.numel(), k)
        if k == "stats":
            _same(view[..., :5], plain[k][..., :5], (k, "differs inside a fenced buffer"))
            _same(view[..., 5:], sent[FENCE:FENCE + view.numel()].view(nA, P, 8)[..., 5:], (k, "stats[5..7] were written"))
        else:
            _same(view, plain[k], (k, "differs inside a fenced buffer"))
    dirty = dict(inp)
    for k in ("old_logp", "adv", "value_preds", "returns", "mask"):
        dirty[k] = inp[k].clone()
        dirty[k][:, rows:] = float("nan")
    for k, v in run_loss(device, dirty, rows, 0, n_parts=n_parts, mask_sum=msum).items():
        assert torch.equal(_bits(v.cpu()), _bits(plain[k].cpu())), (k, "something in [rows, row_stride) was read")
    return {}


def check_prepare_ownership(device, nA=3, bs=1025, T=3):
    """4: the four outputs inside sentinel-filled buffers, and a second launch"""
    ep = make_episodes(nA, bs, T)
    plain = run_prepare(device, ep, "batch", 0, 0)
    for k, v in run_prepare(device, ep, "batch", 0, 0).items():
        _same(v, plain[k], (k, "a second launch differs"))
    fenced = {k: _fenced((nA, bs * T), device) for k in plain}
    run_prepare(device, ep, "batch", 0, 0, outs={k: v[2] for k, v in fenced.items()})
    for k, (sent, buf, view) in fenced.items():
        _fence_intact(sent, buf, view.numel(), k)
        _same(view, plain[k], (k, "differs inside a fenced buffer"))
    return {}


# ================================================================================================ refusals
def check_refusals(device):
    """5: every descriptor the host code rejects comes back as IPLAN_EINVAL with a message that names the entry point; nothing is
    launched, so the sentinel-filled outputs stay as they were; the restored descriptors launch"""
    lib = ops._lib(None)
    EINVAL = _einval()
    nA, rows, bs, T = 2, 6, 3, 2
    stride = rows + 3
    keep = {k: _sentinel(nA * stride, "cpu").view(nA, stride).clone().to(device) for k in
            ("logp", "entropy", "values", "old_logp", "adv", "value_preds", "returns", "mask", "g_logp", "g_values", "stats", "mask_sum", "sum", "sqdev",
             "reward", "values_all", "out_returns", "out_adv", "out_mask", "out_value_preds")}
    keep["terminated"] = torch.zeros(nA * bs * (T + 1), dtype=torch.uint8, device=device)
    before = {k: v.cpu().clone() for k, v in keep.items()}
    p = lambda k: keep[k].data_ptr()  # noqa: E731

    pl = L.PpoLossArgs()
    pl.n_agents, pl.rows, pl.row_stride = nA, rows, stride
    for k in ("logp", "entropy", "values", "old_logp", "adv", "value_preds", "returns", "mask", "g_logp", "g_values", "stats"):
        setattr(pl, k, p(k))
    pl.clip, pl.huber_delta, pl.value_loss_coef = CLIP, HUBER, VCOEF
    pp = L.PpoPrepareArgs()
    pp.n_agents, pp.bs, pp.T = nA, bs, T
    pp.reward, pp.rw_s_net, pp.rw_s_ep, pp.rw_s_t = p("reward"), bs * (T + 1), T + 1, 1
    pp.terminated, pp.tm_s_net, pp.tm_s_ep, pp.tm_s_t = p("terminated"), bs * (T + 1), T + 1, 1
    pp.values, pp.gamma, pp.lam = p("values_all"), GAMMA, LAM
    pp.returns, pp.adv, pp.mask, pp.value_preds = p("out_returns"), p("out_adv"), p("out_mask"), p("out_value_preds")
    an = L.AdvNormArgs()
    an.n_agents, an.n, an.row_stride = nA, rows, stride
    an.adv, an.sum, an.sqdev, an.count, an.phase = p("adv"), p("sum"), p("sqdev"), float(rows), 0
    count = 0

    def refused(name, a, **fields):
        nonlocal count
        fn = getattr(lib.c, name)
        if a is None:
            rc = fn(None, C.c_void_p(0))
        else:
            old = {k: getattr(a, k) for k in fields}
            for k, v in fields.items():
                setattr(a, k, v)
            rc = fn(C.byref(a), C.c_void_p(0))
            for k, v in old.items():
                setattr(a, k, v)
        msg = lib.c.iplan_last_error().decode()
        assert rc == EINVAL and rc < 0 and msg.startswith(name), (name, fields, rc, msg)
        count += 1

    refused("iplan_ppo_loss", None)
    for k in ("logp", "entropy", "values", "old_logp", "adv", "value_preds", "returns", "mask", "g_logp", "g_values", "stats"):
        refused("iplan_ppo_loss", pl, **{k: None})
    refused("iplan_ppo_loss", pl, rows=0)
    refused("iplan_ppo_loss", pl, n_agents=0)
    refused("iplan_ppo_loss", pl, n_parts=2)                                  # n_parts > 1 without mask_sum
    refused("iplan_ppo_loss", pl, n_parts=1025, mask_sum=p("mask_sum"))
    refused("iplan_ppo_loss", pl, rows=stride + 1)                            # rows > row_stride: would read the next agent's rows
    refused("iplan_ppo_loss", pl, rows=stride + 1, n_parts=2, mask_sum=p("mask_sum"))
    refused("iplan_ppo_prepare", None)
    for k in ("reward", "terminated", "values", "returns", "adv", "mask", "value_preds"):
        refused("iplan_ppo_prepare", pp, **{k: None})
    for k in ("n_agents", "bs", "T"):
        refused("iplan_ppo_prepare", pp, **{k: 0})
    refused("iplan_ppo_prepare", pp, bs=1, T=1)                               # bs T < 2: no unbiased std
    refused("iplan_ppo_adv_norm", None)
    for k in ("adv", "sum", "sqdev"):
        refused("iplan_ppo_adv_norm", an, **{k: None})
    refused("iplan_ppo_adv_norm", an, n=0)
    refused("iplan_ppo_adv_norm", an, n_agents=0)
    refused("iplan_ppo_adv_norm", an, phase=-1)
    refused("iplan_ppo_adv_norm", an, phase=3)
    refused("iplan_ppo_adv_norm", an, count=1.0)
    refused("iplan_ppo_adv_norm", an, count=float("nan"))
    refused("iplan_ppo_adv_norm", an, n=stride + 1)                           # n > row_stride: would write the next agent's rows
    _sync(device)
    for k, v in keep.items():
        assert torch.equal(v.cpu(), before[k]), (k, "a refused call wrote something")
    # the restored descriptors launch (rows == row_stride is the edge that stays accepted)
    stream = L.current_stream(device)
    pl.row_stride, an.n = rows, stride
    lib.call("iplan_ppo_loss", pl, stream)
    lib.call("iplan_ppo_prepare", pp, stream)
    lib.call("iplan_ppo_adv_norm", an, stream)
    _sync(device)
    return {"refusals": count}
