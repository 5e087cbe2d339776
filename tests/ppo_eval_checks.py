"""TEST INFRASTRUCTURE: PPO inspection (csrc/ppo_eval.hip, ops.ppo_eval, IPPOLearner.evaluate) on whatever library is active -- the
host emulator in tests/test_emu_ppo_eval.py, the gfx950 build in tests/test_gpu_ppo_eval.py.

Ground truth: the unchanged oracle functions (oracle.normalise_advantages, ppo_losses, and for the method critic_value -> gae_returns
-> normalise_advantages -> actor_evaluate -> ppo_losses) plus the extra statistics written out below, in fp64 torch, with the same
formulas in fp32 torch beside them.  Rule: |got - ref64| / max(1, |ref64|) <= max(1e-5, E32_FACTOR x the fp32
formulas' own error by the same measure), per statistic.  Sum(mask), the live counts and the indicator fractions are exact: the
inputs are built so that no row sits within 1e-4 of a threshold.  The checks never touch ``L.use_library_for_tests``.  Each returns
the worst errors it saw."""
import functools
import os
import re

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import E32_FACTOR, _fields, _Log
from tests.policy_trace_checks import assert_out_refused

TOL = 1e-5
C = L.PPO_EVAL_CHUNK
CLIP = float(np.float32(0.2))           # (the fp32 value the kernel gets, so that fp64 thresholds are the kernel's)
HUBER = 0.75                            # both branches of the Huber loss occur with unit-scale residuals
MARGIN = 1e-4                           # no row closer than this to an indicator's threshold
NAMES, STEP_NAMES = L.PPO_EVAL_STATS, L.PPO_EVAL_STEP_STATS
EXACT = ("mask_sum", "clip_fraction", "value_clip_fraction")
EXACT_STEP = ("count", "clip_fraction")
# (n_agents, bs, T, rows)
SHAPES = [(1, 1, 2, 2), (1, 3, 7, 21), (3, 5, 9, 36), (2, C - 1, 1, C - 1), (2, C, 1, C), (2, C + 1, 1, C + 1), (2, 2 * C + 3, 1, 2 * C + 3)]
FLAG_BITS = (L.PPO_MSE, L.PPO_NO_VCLIP, L.PPO_VALUE_MEAN, L.PPO_POLICY_MEAN)
# (shape, terminated drawn?, flags)
KERNEL_CASES = [(s, masked, 0) for s in SHAPES for masked in (False, True)] + [((3, 5, 9, 36), masked, f) for f in FLAG_BITS for masked in (False, True)]
CASE_IDS = ["x".join(map(str, s)) + ("_terminated" if m else "_all_live") + (f"_flag{f}" if f else "") for s, m, f in KERNEL_CASES]
BIG = (2, 2 * C + 3, 1, 2 * C + 3)
PER_ROW = ("ratio", "adv_norm")
INPUTS = ("logp", "entropy", "values", "old_logp", "adv", "value_preds", "returns", "mask")


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(a, b, what, keys=None):
    for k in (keys or sorted(set(a) & set(b))):
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


# ------------------------------------------------------------------------------------------------ the reference
def flag_kwargs(flags):
    return dict(use_huber_loss=not flags & L.PPO_MSE, use_clipped_value_loss=not flags & L.PPO_NO_VCLIP,
                use_value_active_masks=not flags & L.PPO_VALUE_MEAN, use_policy_active_masks=not flags & L.PPO_POLICY_MEAN)


def reference_agent(dt, logp, ent, values, old_logp, adv_raw, vpred, returns, mask, T, flags, clip=CLIP, huber=HUBER):
    """One agent in dtype ``dt``.  logp / ent / values [rows]; old_logp / vpred / returns / mask [>= rows] (the first ``rows`` are used);
    adv_raw [row_stride], all of it normalised -> dict(stats [16], step [T, 6], ratio [rows], adv_norm [row_stride])"""
    R = logp.shape[0]
    c = lambda t, n=R: t[:n].to(dt).reshape(-1, 1)  # noqa: E731
    logp, ent, values, old_logp, vpred, returns, m = c(logp), c(ent), c(values), c(old_logp), c(vpred), c(returns), c(mask)
    raw = c(adv_raw, adv_raw.shape[0])
    adv_n = O.normalise_advantages(raw, torch.zeros_like(raw), torch.ones_like(raw))     # mean / unbiased std + 1e-5 over ALL entries
    _, pol, _, vloss, ratio = O.ppo_losses(logp, ent.mean(), values, old_logp, adv_n[:R], vpred, returns, m, clip, huber, 0.01, 1.0, **flag_kwargs(flags))
    S = m.sum()
    mmean = lambda x: (m * x).sum() / S  # noqa: E731
    mvar = lambda x: (m * (x - mmean(x)) ** 2).sum() / S  # noqa: E731
    clipped = ((ratio - 1).abs() > clip).to(dt)
    live = ratio[m != 0]
    std, mean = torch.std_mean(raw)
    stats = torch.stack([pol, vloss, ratio.mean(), ent.mean(), S, mmean(old_logp - logp), mmean((ratio - 1) - (logp - old_logp)), mmean(clipped),
                         live.max(), live.min(), 1 - mvar(returns - vpred) / mvar(returns), mmean(((values - vpred).abs() > clip).to(dt)),
                         mean, std, mmean(returns), mmean((returns - values).abs())])
    by = lambda x: x.reshape(-1, T)  # noqa: E731  -- [episodes, T]
    cnt = by(m).sum(0)
    cols = [cnt] + [torch.where(cnt > 0, (by(m) * by(x)).sum(0) / cnt.clamp_min(1), torch.zeros_like(cnt))
                    for x in (raw[:R], (returns - values).abs(), ratio, ent, clipped)]
    return dict(stats=stats, step=torch.stack(cols, -1), ratio=ratio[:, 0], adv_norm=adv_n[:, 0])


def reference(inp, dt, T, flags, rows):
    per = [reference_agent(dt, inp["logp"][i, :rows], inp["entropy"][i, :rows], inp["values"][i, :rows], inp["old_logp"][i], inp["adv"][i],
                           inp["value_preds"][i], inp["returns"][i], inp["mask"][i], T, flags) for i in range(inp["logp"].shape[0])]
    return {k: torch.stack([p[k] for p in per]) for k in per[0]}


def assert_vs_reference(got, r64, r32, worst, what):
    """got: stats [nA, 16], step_stats [nA, T, 6] and optionally ratio / adv_norm; every figure is printed before it is asserted"""
    st, ss = got["stats"].cpu().double(), got["step_stats"].cpu().double()
    for k, name in enumerate(NAMES):
        ref, ref32 = r64["stats"][:, k], r32["stats"][:, k].double()
        if name in EXACT:
            assert torch.equal(got["stats"].cpu()[:, k], ref.float()), (what, name, got["stats"].cpu()[:, k], ref)
            continue
        scale = ref.abs().clamp_min(1.0)
        err, e32 = ((st[:, k] - ref).abs() / scale).max().item(), ((ref32 - ref).abs() / scale).max().item()
        print(what, name, "err", err, "e32", e32)
        _worse(worst, name, err)
        _worse(worst, name + "_e32", e32)
        assert err <= max(TOL, E32_FACTOR * e32), (what, name, err, e32, st[:, k], ref)
    for k, name in enumerate(STEP_NAMES):
        ref, ref32 = r64["step"][..., k], r32["step"][..., k].double()
        if name in EXACT_STEP:
            assert torch.equal(got["step_stats"].cpu()[..., k], ref.float()), (what, "step", name)
            continue
        scale = ref.abs().clamp_min(1.0)
        err, e32 = ((ss[..., k] - ref).abs() / scale).max().item(), ((ref32 - ref).abs() / scale).max().item()
        print(what, "step", name, "err", err, "e32", e32)
        _worse(worst, "step_" + name, err)
        _worse(worst, "step_" + name + "_e32", e32)
        assert err <= max(TOL, E32_FACTOR * e32), (what, "step", name, err, e32)
    dead = r64["step"][..., 0] == 0
    assert torch.equal(got["step_stats"].cpu()[dead], torch.zeros_like(got["step_stats"].cpu()[dead])), (what, "a step nobody lived to is not all zeros")
    for name in PER_ROW:
        if name in got:
            ref = r64[name]
            scale = ref.abs().clamp_min(1.0)
            err, e32 = ((got[name].cpu().double() - ref).abs() / scale).max().item(), ((r32[name].double() - ref).abs() / scale).max().item()
            print(what, name, "err", err, "e32", e32)
            _worse(worst, name, err)
            _worse(worst, name + "_e32", e32)
            assert err <= max(TOL, E32_FACTOR * e32), (what, name, err, e32)


# ------------------------------------------------------------------------------------------------ synthetic per-row inputs
@functools.lru_cache(maxsize=None)
def make_inputs(shape, masked, seed=0, same_logp=False):
    """fp32 host tensors of one case, never modified.  logp - old_logp ~ N(0, 0.2^2); no row within MARGIN of the ratio's or the value
    clip's threshold; masked: terminated ~ Bernoulli(0.3) with >= 2 live rows per agent and EXACTLY 2 for the last agent, one of
    them clipped and one not; a step with nobody alive for agent 0 where T >= 3.  Conditions on the inputs, checked on the fp64
    reference: every agent has a clipped and an unclipped live row."""
    nA, bs, T, rows = shape
    stride = bs * T
    for attempt in range(200):
        gen = torch.Generator().manual_seed(1000 * seed + 7 * attempt + sum(shape) + (500 if masked else 0))
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        logp = -1.2 + 0.5 * rnd(nA, stride)
        delta = 0.2 * rnd(nA, stride)
        values = rnd(nA, stride)
        dv = 0.25 * rnd(nA, stride)
        for _ in range(50):                                                        # redraw the rows next to a threshold
            old = logp - delta
            near = ((torch.exp(logp.double() - old.double()) - 1).abs() - CLIP).abs() < 2 * MARGIN
            vp = values - dv
            near_v = ((values.double() - vp.double()).abs() - CLIP).abs() < 2 * MARGIN
            if not (near.any() or near_v.any()):
                break
            delta = torch.where(near, 0.2 * rnd(nA, stride), delta)
            dv = torch.where(near_v, 0.25 * rnd(nA, stride), dv)
        else:
            continue
        if same_logp:
            old = logp.clone()
        returns = values + rnd(nA, stride)
        entropy = 0.2 + 1.4 * torch.rand(nA, stride, generator=gen)
        clipped = (torch.exp(logp.double() - old.double()) - 1).abs() > CLIP
        mask = torch.ones(nA, stride)
        if masked:
            mask = (torch.rand(nA, stride, generator=gen) >= 0.3).float()
            if T >= 3:
                mask.view(nA, bs, T)[0, :, T - 1] = 0
            for i in range(nA):
                if mask[i, :rows].sum() < 2:
                    mask[i, :2] = 1
            if not same_logp:
                c_idx, u_idx = torch.nonzero(clipped[-1, :rows]), torch.nonzero(~clipped[-1, :rows])
                if len(c_idx) == 0 or len(u_idx) == 0:
                    continue
                mask[-1, :rows] = 0
                mask[-1, c_idx[0]] = 1
                mask[-1, u_idx[0]] = 1
            else:
                mask[-1, :rows] = 0
                mask[-1, :2] = 1
        live = mask[:, :rows] != 0
        if not same_logp and not all((clipped[i, :rows] & live[i]).any() and (~clipped[i, :rows] & live[i]).any() for i in range(nA)):
            continue
        adv = (returns - vp) * mask                                               # what iplan_ppo_prepare(skip_norm = 1) leaves
        inp = dict(logp=logp[:, :rows].contiguous(), entropy=entropy[:, :rows].contiguous(), values=values[:, :rows].contiguous(), old_logp=old,
                   adv=adv, value_preds=vp, returns=returns, mask=mask)
        # the conditions, on the reference
        r = torch.exp(inp["logp"].double() - old[:, :rows].double())
        assert (((r - 1).abs() - CLIP).abs() >= MARGIN).all() or same_logp
        assert (((inp["values"].double() - vp[:, :rows].double()).abs() - CLIP).abs() >= MARGIN).all()
        assert (live.sum(1) >= 2).all() and (not masked or live[-1].sum() == 2)
        if not same_logp:
            for i in range(nA):
                hit = (r[i] - 1).abs() > CLIP
                assert (hit & live[i]).any() and (~hit & live[i]).any(), ("inputs", shape, masked, i)
        return inp
    raise AssertionError(("no admissible draw", shape, masked))


@functools.lru_cache(maxsize=None)
def _reference(shape, masked, flags, dt, seed=0, same_logp=False):
    return reference(make_inputs(shape, masked, seed, same_logp), dt, shape[2], flags, shape[3])


def run(inp, device, T, rows, flags=0, n_parts=0, want=PER_ROW, out=None):
    d = {k: v.to(device) for k, v in inp.items()}
    res = ops.ppo_eval(*(d[k] for k in INPUTS), T, rows=rows, clip=CLIP, huber_delta=HUBER, flags=flags, n_parts=n_parts, want=want, out=out)
    _sync(device)
    return res


# ------------------------------------------------------------------------------------------------ the kernel alone
def check_kernel(device, shape, masked, flags):
    """1: every statistic, per-step statistic and per-row output against fp64"""
    worst = {}
    got = run(make_inputs(shape, masked), device, shape[2], shape[3], flags)
    assert_vs_reference(got, _reference(shape, masked, flags, torch.float64), _reference(shape, masked, flags, torch.float32), worst, (shape, masked, flags))
    return worst


def check_parts(device):
    """2: n_parts in {1, 2, 7, 64} at rows = 2 C + 3: identical bits on every output"""
    inp = make_inputs(BIG, True)
    first = run(inp, device, BIG[2], BIG[3], n_parts=1)
    for parts in (2, 7, 64):
        assert_same_bits(run(inp, device, BIG[2], BIG[3], n_parts=parts), first, ("n_parts", parts), ("stats", "step_stats") + PER_ROW)
    return {}


def check_repeatable(device, reps):
    """3: ``reps`` launches on the same inputs: identical bits"""
    inp = make_inputs(BIG, True)
    first = run(inp, device, BIG[2], BIG[3], n_parts=7)
    for _ in range(reps - 1):
        assert_same_bits(run(inp, device, BIG[2], BIG[3], n_parts=7), first, "repeat", ("stats", "step_stats") + PER_ROW)
    return {}


def _sentinels(shape, device, shift=0.0):
    nA, bs, T, rows = shape
    shapes = dict(stats=(nA, len(NAMES)), step_stats=(nA, T, len(STEP_NAMES)), ratio=(nA, rows), adv_norm=(nA, bs * T))
    bufs = {}
    for k, s in shapes.items():
        n = int(np.prod(s))
        sent = 0.5 + shift + (torch.arange(n + 64, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        bufs[k] = (sent, buf, buf[32:32 + n].view(s))
    return bufs


def check_sentinel(device, shape=(3, 5, 9, 36)):
    """4: outputs carved out of sentinel-filled buffers: nothing outside an output's extent is written, every element inside is, and
    an optional output that was not asked for is left alone"""
    inp = make_inputs(shape, True)
    ref = run(inp, device, shape[2], shape[3])
    for want in (PER_ROW, ("ratio",), ()):
        bufs = _sentinels(shape, device)
        got = run(inp, device, shape[2], shape[3], want=want, out={k: v[2] for k, v in bufs.items() if k in ("stats", "step_stats") + tuple(want)})
        assert set(got) == {"stats", "step_stats"} | set(want)
        for k, (sent, buf, view) in bufs.items():
            host = buf.cpu()
            if k not in got:
                assert torch.equal(host, sent), (k, "was not asked for and was written")
                continue
            assert got[k].data_ptr() == view.data_ptr()
            assert torch.equal(_bits(view), _bits(ref[k])), (k, "differs inside a padded buffer")
            n = view.numel()
            assert torch.equal(host[:32], sent[:32]) and torch.equal(host[32 + n:], sent[32 + n:]), (k, "an element outside the extent was written")
    b2 = _sentinels(shape, device, 0.25)                      # every element is written: a second, shifted sentinel ends the same
    run(inp, device, shape[2], shape[3], out={k: v[2] for k, v in b2.items()})
    for k in b2:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (k, "an element was left unwritten")
    return {}


def check_poison(device, shape=(3, 5, 9, 36)):
    """5: NaN in everything beyond ``rows`` (old_logp, value_preds, returns, mask; adv is read over all bs T entries): finite
    statistics, same bits"""
    nA, bs, T, rows = shape
    assert rows < bs * T
    inp = make_inputs(shape, True)
    dirty = dict(inp)
    for k in ("old_logp", "value_preds", "returns", "mask"):
        dirty[k] = inp[k].clone()
        dirty[k][:, rows:] = float("nan")
    a, b = run(inp, device, T, rows, n_parts=2), run(dirty, device, T, rows, n_parts=2)
    for k in ("stats", "step_stats") + PER_ROW:
        assert torch.isfinite(b[k]).all(), (k, "not finite")
    assert_same_bits(a, b, "read something beyond its rows")
    return {}


def check_identity(device, shape=(3, 5, 9, 36)):
    """6: old_logp == logp: ratio == 1, both KLs == 0 and the clip fraction == 0 exactly"""
    for masked in (False, True):
        inp = make_inputs(shape, masked, same_logp=True)
        got = run(inp, device, shape[2], shape[3])
        st = {n: got["stats"][:, k].cpu() for k, n in enumerate(NAMES)}
        assert torch.equal(got["ratio"].cpu(), torch.ones_like(got["ratio"].cpu()))
        for n, v in (("ratio_mean", 1.0), ("ratio_max", 1.0), ("ratio_min", 1.0), ("approx_kl", 0.0), ("approx_kl_k3", 0.0), ("clip_fraction", 0.0)):
            assert torch.equal(st[n], torch.full_like(st[n], v)), (n, st[n])
        ss = got["step_stats"].cpu()
        assert torch.equal(ss[..., 5], torch.zeros_like(ss[..., 5])) and torch.equal(ss[..., 3], (ss[..., 0] > 0).float())
    return {}


def _prepare(device, nA, bs, T, seed, skip_norm):
    gen = torch.Generator().manual_seed(seed)
    reward = torch.randn(bs, T + 1, nA, 1, generator=gen)
    term = (torch.rand(bs, T + 1, nA, 1, generator=gen) < 0.2).to(torch.uint8)
    v_all = torch.randn(nA, bs, T + 1, generator=gen)
    rw, tm, va = reward.to(device), term.to(device), v_all.to(device)
    pp = L.PpoPrepareArgs()
    pp.n_agents, pp.bs, pp.T = nA, bs, T
    pp.reward, pp.rw_s_net, pp.rw_s_ep, pp.rw_s_t = rw.data_ptr(), rw.stride(2), rw.stride(0), rw.stride(1)
    pp.terminated, pp.tm_s_net, pp.tm_s_ep, pp.tm_s_t = tm.data_ptr(), tm.stride(2), tm.stride(0), tm.stride(1)
    pp.values, pp.gamma, pp.lam = va.data_ptr(), 0.99, 0.95
    outs = [torch.empty(nA, bs * T, device=device) for _ in range(4)]
    pp.returns, pp.adv, pp.mask, pp.value_preds = (o.data_ptr() for o in outs)
    pp.skip_norm = skip_norm
    ops._lib(None).call("iplan_ppo_prepare", pp, L.current_stream(device))
    _sync(device)
    return dict(zip(("returns", "adv", "mask", "value_preds"), outs))


def check_agrees_with_prepare(device, shape=(3, 5, 9, 36)):
    """7: adv_norm against what iplan_ppo_prepare(skip_norm = 0) writes on the same rewards / values: each within the bound of the
    fp64 normalisation of the raw advantage, their distance within the sum of the two bounds"""
    nA, bs, T, rows = shape
    raw, normed = _prepare(device, nA, bs, T, 5, 1), _prepare(device, nA, bs, T, 5, 0)
    assert_same_bits(raw, normed, "prepare", ("returns", "mask", "value_preds"))
    inp = dict(make_inputs(shape, False))
    inp.update({k: v.cpu() for k, v in raw.items()})
    got = run(inp, device, T, rows, want=("adv_norm",))["adv_norm"].cpu().double()
    worst = {}
    for i in range(nA):
        r64, r32 = (O.normalise_advantages(x, torch.zeros_like(x), torch.ones_like(x)) for x in (inp["adv"][i].double(), inp["adv"][i]))
        scale = r64.abs().clamp_min(1.0)
        e32 = ((r32.double() - r64).abs() / scale).max().item()
        bound = max(TOL, E32_FACTOR * e32)
        e_eval, e_prep = ((got[i] - r64).abs() / scale).max().item(), ((normed["adv"][i].cpu().double() - r64).abs() / scale).max().item()
        between = ((got[i] - normed["adv"][i].cpu().double()).abs() / scale).max().item()
        print("adv_norm agent", i, "eval", e_eval, "prepare", e_prep, "between", between, "e32", e32)
        for k, v in (("adv_norm_eval", e_eval), ("adv_norm_prepare", e_prep), ("adv_norm_between", between), ("adv_norm_e32", e32)):
            _worse(worst, k, v)
        assert e_eval <= bound and e_prep <= bound and between <= 2 * bound, (i, e_eval, e_prep, between, e32)
    return worst


def _ppo_loss(device, inp, adv_norm, rows, flags):
    d = {k: v.to(device).contiguous() for k, v in inp.items()}
    nA, stride = d["old_logp"].shape
    pl = L.PpoLossArgs()
    pl.n_agents, pl.rows, pl.row_stride = nA, rows, stride
    pl.logp, pl.entropy, pl.values = d["logp"].data_ptr(), d["entropy"].data_ptr(), d["values"].data_ptr()
    pl.old_logp, pl.adv, pl.value_preds = d["old_logp"].data_ptr(), adv_norm.data_ptr(), d["value_preds"].data_ptr()
    pl.returns, pl.mask = d["returns"].data_ptr(), d["mask"].data_ptr()
    pl.clip, pl.huber_delta, pl.value_loss_coef, pl.flags = CLIP, HUBER, 1.0, flags
    g1, g2, stats = torch.empty(nA, rows, device=device), torch.empty(nA, rows, device=device), torch.zeros(nA, 8, device=device)
    pl.g_logp, pl.g_values, pl.stats = g1.data_ptr(), g2.data_ptr(), stats.data_ptr()
    ops._lib(None).call("iplan_ppo_loss", pl, L.current_stream(device))
    _sync(device)
    return stats[:, :5].cpu().double()


def check_agrees_with_loss(device, shape=(3, 5, 9, 36)):
    """8: stats 0-4 against iplan_ppo_loss's five on the same inputs (the loss kernel gets this kernel's normalised advantages): each
    within the bound of fp64, their distance within the sum of the two bounds"""
    worst = {}
    for flags in (0,) + FLAG_BITS:
        inp = make_inputs(shape, True)
        got = run(inp, device, shape[2], shape[3], flags, want=("adv_norm",))
        loss = _ppo_loss(device, inp, got["adv_norm"], shape[3], flags)
        r64, r32 = _reference(shape, True, flags, torch.float64), _reference(shape, True, flags, torch.float32)
        for k in range(5):
            ref = r64["stats"][:, k]
            scale = ref.abs().clamp_min(1.0)
            e32 = ((r32["stats"][:, k].double() - ref).abs() / scale).max().item()
            bound = max(TOL, E32_FACTOR * e32)
            e_eval, e_loss = ((got["stats"][:, k].cpu().double() - ref).abs() / scale).max().item(), ((loss[:, k] - ref).abs() / scale).max().item()
            between = ((got["stats"][:, k].cpu().double() - loss[:, k]).abs() / scale).max().item()
            print("flags", flags, NAMES[k], "eval", e_eval, "loss", e_loss, "between", between, "e32", e32)
            _worse(worst, NAMES[k] + "_between", between)
            _worse(worst, NAMES[k] + "_loss_kernel", e_loss)
            assert e_eval <= bound and e_loss <= bound and between <= 2 * bound, (flags, NAMES[k], e_eval, e_loss, between, e32)
    return worst


def _einval():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iplan_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(IPLAN_E\w+)\s*=\s*(-?\d+)", text)}["IPLAN_EINVAL"]


def check_bad_arguments(device, shape=(3, 5, 9, 36)):
    """9: each invalid descriptor is refused by the host-side check with IPLAN_EINVAL and a message; an ``out=`` destination of the wrong
    shape or dtype, or a non-contiguous one, makes ops.ppo_eval raise AssertionError; nothing is launched, so the sentinel-filled outputs
    stay as they were"""
    nA, bs, T, rows = shape
    inp = make_inputs(shape, True)
    good = run(inp, device, T, rows)
    lib = ops._lib(None)
    d = {k: v.to(device) for k, v in inp.items()}
    bufs = _sentinels(shape, device)
    a, res, keep = ops.ppo_eval_args(*(d[k] for k in INPUTS), T, rows=rows, clip=CLIP, huber_delta=HUBER, want=PER_ROW,
                                     out={k: v[2] for k, v in bufs.items()})
    EINVAL = _einval()
    fn = lib.c.iplan_ppo_eval

    def refused(args_ref, **fields):
        before = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        rc = fn(args_ref, L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, v in before.items():
            setattr(a, k, v)
        assert rc == EINVAL and rc < 0 and "iplan_ppo_eval" in msg, (fields, rc, msg)

    refused(None)
    ref = L.C.byref(a)
    refused(ref, rows=bs * T + T)                             # rows > row_stride
    refused(ref, rows=rows - 1)                               # not a multiple of T
    refused(ref, n_agents=0)
    refused(ref, T=0)
    for k in INPUTS + ("stats", "step_stats", "workspace"):
        refused(ref, **{k: None})
    assert_out_refused(lambda out: ops.ppo_eval(*(d[k] for k in INPUTS), T, rows=rows, clip=CLIP, huber_delta=HUBER, want=PER_ROW, out=out),
                       bufs, ("stats", "step_stats", "ratio"))
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(buf.cpu(), sent), (k, "a refused call wrote an output")
    assert_same_bits(run(inp, device, T, rows), good, "after the refusals")
    del keep, res
    return {}


# ------------------------------------------------------------------------------------------------ the method
def _small_args(device, **kw):
    from iplan_amd.config import default_args
    base = dict(use_cuda=torch.device(device).type == "cuda", max_vehicle_num=4, n_agents=2, episode_limit=4, batch_size_run=3, max_history_len=3,
                pred_batch_size=6, pred_length=2, buffer_size=3, batch_size=3, ppo_epoch=1)
    base.update(kw)
    return default_args("highway", **base)


def _make(args, seed, spread=True):
    from iplan_amd import synth
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    from iplan_amd.learners.ippo_learner import IPPOLearner
    torch.manual_seed(seed)
    scheme = synth.make_scheme(args)
    mac = DcntrlMAC(scheme, {"agents": args.n_agents}, args)
    if spread:                                                # (the default initialisation leaves the heads near zero)
        gen = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for m in mac.agents + mac.critics:
                for p in m.parameters():
                    p.add_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return mac, IPPOLearner(mac, scheme, _Log(), args), scheme


def _snapshot(mac, scheme, args):
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    snap = DcntrlMAC(scheme, {"agents": args.n_agents}, args)
    for dst, src in zip(snap.agents + snap.critics, mac.agents + mac.critics):
        dst.load_state_dict(src.state_dict())
    return snap


def _params(mac, dt):
    conv = lambda m: {k: v.detach().cpu().to(dt) for k, v in m.state_dict().items()}  # noqa: E731
    return [conv(m) for m in mac.agents], [conv(m) for m in mac.critics]


def method_reference(mac, old, f, args, dt):
    """the oracle chain of every agent in ``dt``: critic_value (old's critics) -> gae_returns -> normalise_advantages -> actor_evaluate
    (old's actors: old log-probs; the learner's: logp, entropy) -> critic_value (the learner's) -> ppo_losses + the extra statistics"""
    nA, n_act = args.n_agents, args.n_actions
    E, T1 = f["history"].shape[:2]
    T = T1 - 1
    ap, cp = _params(mac, dt)
    oap, ocp = _params(old, dt)
    flags = ((0 if args.use_huber_loss else L.PPO_MSE) | (0 if args.use_clipped_value_loss else L.PPO_NO_VCLIP)
             | (0 if args.use_value_active_masks else L.PPO_VALUE_MEAN) | (0 if args.use_policy_active_masks else L.PPO_POLICY_MEAN))
    per, rowsets = [], []
    for i in range(nA):
        x_all = O.build_inputs_train(i, f["history"][:, :, i].to(dt), f["attention_latent"][:, :, i].to(dt), f["behavior_latent"][:, :, i].to(dt),
                                     f["actions_onehot"][:, :, i], nA, args.GAT_enable, args.Behavior_enable)
        F_ = x_all.shape[-1]
        masks_all = 1.0 - f["terminated"][:, :, i].to(dt)
        hc_all = f["rnn_states_critics"][:, :, i].to(dt)
        M = hc_all.shape[-1]
        v_all, _ = O.critic_value(ocp[i], x_all.reshape(-1, F_), hc_all.reshape(-1, M), use_relu=args.use_ReLU)
        v_all = v_all.reshape(E, T1, 1)
        rets = O.gae_returns(f["reward"][:, :-1, i].to(dt), v_all, masks_all, args.gamma, args.gae_lambda, args.use_gae)
        m = masks_all[:, :-1]
        raw = (rets - v_all[:, :-1]).clone()
        raw[m == 0.0] = 0.0
        x = x_all[:, :-1].reshape(-1, F_)
        ha, hc = f["rnn_states_actors"][:, :-1, i].to(dt).reshape(-1, M), hc_all[:, :-1].reshape(-1, M)
        acts, avail = f["actions"][:, :-1, i].reshape(-1, 1), f["avail_actions"][:, :-1, i].reshape(-1, n_act)
        old_logp, _ = O.actor_evaluate(oap[i], x, ha, acts, avail, use_relu=args.use_ReLU)
        logp, ent_mean = O.actor_evaluate(ap[i], x, ha, acts, avail, use_relu=args.use_ReLU)
        la = torch.log_softmax(O.actor_logits(ap[i], x, ha, avail, use_relu=args.use_ReLU)[0], -1)
        ent = -(la.exp() * la.clamp_min(torch.finfo(dt).min)).sum(-1)
        assert torch.allclose(ent.mean(), ent_mean)
        val, _ = O.critic_value(cp[i], x, hc, use_relu=args.use_ReLU)
        r = reference_agent(dt, logp[:, 0], ent, val[:, 0], old_logp[:, 0], raw.reshape(-1), v_all[:, :-1].reshape(-1), rets.reshape(-1), m.reshape(-1),
                            T, flags, clip=float(np.float32(args.clip_param)), huber=args.huber_delta)
        # (the unbiased normaliser of this chain is O.normalise_advantages on the returns and values themselves: the same numbers)
        assert torch.allclose(r["adv_norm"].reshape(E, T, 1), O.normalise_advantages(rets, v_all[:, :-1], m), rtol=1e-4, atol=1e-5)
        per.append(r)
        rowsets.append(dict(values=v_all[..., 0], returns=rets[..., 0], advantages=r["adv_norm"].reshape(E, T), advantages_raw=raw[..., 0],
                            logp=logp.reshape(E, T), ratio=r["ratio"].reshape(E, T), mask=m[..., 0]))
    out = {k: torch.stack([p[k] for p in per]) for k in per[0]}
    out["rows"] = {k: torch.stack([rs[k] for rs in rowsets], -1) for k in rowsets[0]}                  # [E, T(+1), nA]
    return out


def _as_kernel_result(ev):
    return dict(stats=torch.as_tensor(np.stack([ev[n] for n in NAMES], -1)), step_stats=torch.as_tensor(ev["per_step"]))


def _state(learner, batch):
    from iplan_amd.optim import _moments
    mac = learner.mac
    tensors = [mac.actor_arena.data, mac.critic_arena.data, mac.actor_arena.grad, mac.critic_arena.grad, *_moments(mac.actor_arena), *_moments(mac.critic_arena)]
    tensors += [v for _, v in sorted(learner.store.data.items())] + [v for _, v in sorted(batch.data.items())]
    return [t.clone() for t in tensors], tensors


def check_method(device, E=3):
    """10: evaluate(batch) and evaluate(batch, old=snapshot) against the fp64 chain; evaluate just before a one-epoch train()
    against that train()'s logged losses; the part-filled store; what the call must leave alone; the argument errors"""
    dev_t = torch.device(device).type
    args = _small_args(device, buffer_size=4)
    mac, learner, scheme = _make(args, 31)
    nA, T, T1 = args.n_agents, args.episode_limit, args.episode_limit + 1
    f, batch = _fields(args, E, 9, 0.2, device)
    worst = {}
    # ---- what it must leave alone
    learner.batch_size_run = E
    learner.insert_episode_batch(batch)                       # 3 of 4 episodes: train() would refuse
    assert learner.store.count == E < learner.store.size and not learner.buffers[0].can_sample()
    mac.hidden_states = "untouched"
    learner.last_train_info = "untouched"
    before, live = _state(learner, batch)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state() if dev_t == "cuda" else None, np.random.get_state())
    ev = learner.evaluate(batch, want=learner.EVAL_ROW_TENSORS)
    ev_store = learner.evaluate()
    ev_np = learner.evaluate({k: v.numpy() for k, v in f.items()}, want=("ratio", "values"))
    _sync(device)
    assert torch.equal(torch.get_rng_state(), rng[0]) and (rng[1] is None or torch.equal(torch.cuda.get_rng_state(), rng[1]))
    now = np.random.get_state()
    assert now[0] == rng[2][0] and np.array_equal(now[1], rng[2][1]) and now[2:] == rng[2][2:]
    for b, t in zip(before, live):
        assert torch.equal(b.view(torch.uint8) if b.dtype != torch.uint8 else b, t.view(torch.uint8) if t.dtype != torch.uint8 else t), "evaluate wrote something"
    assert learner.store.count == E and mac.hidden_states == "untouched" and learner.last_train_info == "untouched"
    # ---- shapes, containers, the store and the numpy batch give the batch's bits
    for n in NAMES:
        assert isinstance(ev[n], np.ndarray) and ev[n].shape == (nA,) and ev[n].dtype == np.float32, n
        assert np.array_equal(ev[n], ev_store[n], equal_nan=True) and np.array_equal(ev[n], ev_np[n], equal_nan=True), n
    assert ev["per_step"].shape == (nA, T, 6) and np.array_equal(ev["per_step"], ev_store["per_step"])
    for k in learner.EVAL_ROW_TENSORS:
        assert torch.is_tensor(ev[k]) and ev[k].device.type == dev_t and ev[k].shape == (E, T1 if k == "values" else T, nA), (k, ev[k].shape)
    assert isinstance(ev_np["ratio"], np.ndarray) and np.array_equal(ev_np["ratio"], ev["ratio"].cpu().numpy()) and ev_np["values"].shape == (E, T1, nA)
    assert set(ev_store) == set(NAMES) | {"per_step"}
    two = learner.evaluate(batch, episodes=2)
    assert two["per_step"].shape == (nA, T, 6) and (two["mask_sum"] <= ev["mask_sum"]).all() and (two["per_step"][..., 0] <= 2).all()
    # ---- old = None: the chain with the learner's own nets on both sides
    r64, r32 = (method_reference(mac, mac, f, args, dt) for dt in (torch.float64, torch.float32))
    assert_vs_reference(_as_kernel_result(ev), r64, r32, worst, "evaluate(batch)")
    for n, v in (("ratio_mean", 1.0), ("approx_kl", 0.0), ("approx_kl_k3", 0.0), ("clip_fraction", 0.0)):
        assert np.array_equal(ev[n], np.full(nA, v, np.float32)), (n, ev[n])
    for k in learner.EVAL_ROW_TENSORS:
        ref = r64["rows"][k]
        scale = ref.abs().clamp_min(1.0)
        err, e32 = ((ev[k].cpu().double() - ref).abs() / scale).max().item(), ((r32["rows"][k].double() - ref).abs() / scale).max().item()
        print("evaluate(batch) rows", k, "err", err, "e32", e32)
        _worse(worst, "rows_" + k, err)
        _worse(worst, "rows_" + k + "_e32", e32)
        assert err <= max(TOL, E32_FACTOR * e32), (k, err, e32)
    # ---- old_logp override; the argument errors
    shifted = ev["logp"] - 0.05
    over = learner.evaluate(batch, old_logp=shifted.cpu().numpy())
    assert np.allclose(over["ratio_mean"], np.exp(0.05), rtol=1e-5) and np.allclose(over["approx_kl"], -0.05, atol=1e-5)
    assert np.array_equal(over["value_loss"], ev["value_loss"])
    for bad in (lambda: learner.evaluate(batch, old=mac, old_logp=shifted), lambda: learner.evaluate(batch, want=("nope",))):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a ValueError was expected")
    learner.dp = object()
    try:
        learner.evaluate(batch)
    except NotImplementedError:
        pass
    else:
        raise AssertionError("a data-parallel learner must refuse")
    learner.dp = None
    return worst


def check_method_vs_train(device, E=3):
    """11: evaluate() on the full store just before a one-epoch train() reproduces that train()'s logged value_loss, policy_loss,
    dist_entropy and ratio within 1e-5; then, with the nets one step away from the snapshot, evaluate(batch, old=snapshot) against
    the fp64 chain whose returns / advantages / value_preds / old log-probs come from the snapshot's nets, and a positive KL"""
    args = _small_args(device)
    mac, learner, scheme = _make(args, 37)
    f, batch = _fields(args, E, 11, 0.2, device)
    learner.batch_size_run = E
    learner.insert_episode_batch(batch)
    assert learner.buffers[0].can_sample()
    snap = _snapshot(mac, scheme, args)
    ev = learner.evaluate()
    learner.train(0)
    _sync(device)
    info = learner.last_train_info
    worst = {}
    for name in ("value_loss", "policy_loss", "dist_entropy", "ratio"):
        got, ref = float(np.mean(ev["ratio_mean" if name == "ratio" else name].astype(np.float64))), info[name]
        err = abs(got - ref) / max(1.0, abs(ref))
        print("evaluate before train", name, got, ref, "err", err)
        _worse(worst, "train_" + name, err)
        assert err <= 1e-5, (name, got, ref)
    assert not torch.equal(mac.actor_arena.data, snap.actor_arena.data) and not torch.equal(mac.critic_arena.data, snap.critic_arena.data)
    moved = learner.evaluate(batch, old=snap)
    r64, r32 = (method_reference(mac, snap, f, args, dt) for dt in (torch.float64, torch.float32))
    assert_vs_reference(_as_kernel_result(moved), r64, r32, worst, "evaluate(batch, old=snapshot)")
    print("approx_kl", moved["approx_kl"], "approx_kl_k3", moved["approx_kl_k3"])
    assert (moved["approx_kl_k3"] > 0).all() and (r64["stats"][:, 6] > 0).all(), moved["approx_kl_k3"]
    assert (moved["ratio_max"] > moved["ratio_min"]).all()
    return worst


def check_train_unaffected(device):
    """12: train() gives the same parameters, bit for bit, whether or not evaluate() ran between the insert and the train"""
    args = _small_args(device, episode_limit=9, buffer_size=4, batch_size=3, batch_size_run=3, ppo_epoch=2, max_vehicle_num=5)
    results = []
    for with_eval in (False, True):
        mac, learner, _ = _make(args, 6, spread=False)
        E = args.buffer_size
        _, batch = _fields(args, E, 7, 0.15, device)
        learner.batch_size_run = E
        learner.insert_episode_batch(batch)
        torch.manual_seed(83)
        if with_eval:
            ev = learner.evaluate(want=("advantages",))
            assert np.isfinite(ev["policy_loss"]).all() and torch.isfinite(ev["advantages"]).all()
        learner.train(0)
        _sync(device)
        results.append((mac.actor_arena.data.clone(), mac.critic_arena.data.clone(), dict(learner.last_train_info)))
    (a0, c0, i0), (a1, c1, i1) = results
    assert torch.equal(_bits(a0), _bits(a1)) and torch.equal(_bits(c0), _bits(c1)) and i0 == i1
    return {}
