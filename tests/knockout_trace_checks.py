"""TEST INFRASTRUCTURE: policy knock-out through time (csrc/policy_knockout_trace.hip, ops.policy_knockout_trace,
DcntrlMAC.knockout_trace) on whatever library is active -- the host emulator in tests/test_emu_knockout_trace.py, the gfx950 build in
tests/test_gpu_knockout_trace.py.

Cases are (nA, E, S, N, d, n_actions), J, (start, D, H) on policy_knockout_checks.Case (a batch of S + 1 steps).
Ground truth 1 (bits): job j against the trace of the same nets on an explicit copy of the batch with entity j's columns replaced in
steps start .. start + D - 1 only, from the same start state.  The public ``policy_trace`` always starts at step 0, where there is no
last action; a window with start > 0 takes the recorded action of start - 1, so the window is traced with ``DcntrlMAC._trace(copy,
start, H, hidden0, ...)``, the function ``policy_trace`` and ``action_distribution`` are made of -- and, where start = 0, with the
public ``policy_trace(..., return_hidden=True)`` on the copy sliced to the window as well.
Ground truth 2 (fp64): policy_trace_checks._method_reference, the fp64 oracle chain, on the modified fields.  Rule: error
= max|got - ref64| / max(1, max|ref64|) per agent and tensor, bound = max(1e-5, E32_FACTOR x the fp32 oracle's own distance from fp64).
Left out, as in policy_knockout_checks: logp of rows with no available action; the KL floor (the comparison is not vacuous: some knocked
pair of every agent has fp64 KL > 1e-6) is asked of pairs with two available actions or more.  Each check returns the worst errors it saw."""
import copy
import os

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from tests import saliency_checks as SC
from tests.oracle_checks import E32_FACTOR, _rel
from tests.policy_knockout_checks import GAP, KL_FLOOR, SKIP_CAP, _baseline, _case, get_case, job_list
from tests.policy_trace_checks import _bits, _codes, _method_reference, _sync, _worse, make_mac

TOL = 1e-5
M = 64
ALL_WANT = ("kl", "probs_ko", "logp_ko", "values_ko", "h_actor_ko", "h_critic_ko")
PAIR_KEYS = ("kl", "dlogp", "dvalue", "greedy", "flip", "state_shift_actor", "state_shift_critic", "probs_ko", "logp_ko", "values_ko", "h_actor_ko",
             "h_critic_ko")
BASE_KEYS = ("logp", "values", "probs", "target_action", "greedy_base")
OP_WANT = ("base", "kl", "dlogp", "dvalue", "greedy_ko", "shift_sq", "probs_ko", "logp_ko", "values_ko", "h_ko", "logp_all_ko")

BIT_CASES = [
    ((1, 1, 1, 2, 5, 5), 1, (0, 1, 1), {}),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), {}),
    ((1, 2, 4, 3, 5, 5), 4, (0, 4, 4), {}),
    ((1, 1, 4, 3, 5, 5), 3, (3, 1, 1), {}),
    ((1, 2, 3, 17, 5, 5), 15, (0, 2, 3), {}),
    ((1, 2, 3, 17, 5, 5), 16, (0, 2, 3), {}),
    ((1, 2, 3, 17, 5, 5), 17, (0, 2, 3), {}),
    ((1, 2, 3, 17, 5, 5), 33, (0, 2, 3), {}),
    ((5, 1, 3, 3, 5, 5), 4, (0, 1, 3), {}),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), dict(which="actor")),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), dict(which="critic")),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), dict(tanh=True)),
    ((1, 2, 4, 3, 5, 5), 4, (1, 2, 3), dict(gat=False)),
    ((1, 2, 4, 3, 5, 5), 4, (1, 2, 3), dict(beh=False)),
    ((1, 2, 4, 3, 5, 5), 4, (1, 2, 3), dict(gat=False, beh=False)),
    ((2, 2, 4, 3, 5, 1), 4, (1, 1, 3), {}),
]
BIT_IDS = ["smallest", "pulse_echo2", "throughout_from0", "last_step", "N17_J15", "N17_J16", "N17_J17", "N17_J33", "five_nets", "actor_only",
           "critic_only", "tanh", "no_gat", "no_beh", "history_only", "one_action"]
FP64_CASES = [BIT_CASES[i] for i in (1, 2, 6, 8, 9, 10, 11, 14, 15)]
FP64_IDS = [BIT_IDS[i] for i in (1, 2, 6, 8, 9, 10, 11, 14, 15)]
DIMS = (2, 2, 4, 3, 5, 5)                  # the case of the checks that need no special shape
WIN = (1, 1, 3)


def window_fields(case, j, start, D, sources=None, baseline=None, fields=None):
    """a copy of the episode fields with entity j's columns of ``sources`` replaced in steps start .. start + D - 1 (j = -1: a plain copy)"""
    f = {k: v.clone() for k, v in (fields or case.f).items()}
    if j >= 0:
        for k in (case.names if sources is None else sources):
            f[k][:, start:start + D, :, j] = 0.0 if baseline is None or baseline.get(k) is None else baseline[k].to(f[k].dtype)
    return f


def run(case, win, batch=None, **kw):
    start, D, H = win
    res = case.mac.knockout_trace(case.batch if batch is None else batch, start=start, duration=D, horizon=H, **kw)
    _sync(case.device)
    return res


def window_trace(case, f, start, H, which="both", hidden0=None):
    """the nets' own trace over the window of fields ``f`` -> [E, H, nA, ..] probs, greedy, logp, values, h_actor, h_critic"""
    res, _, _ = case.mac._trace(case.to_batch(f), start, H, hidden0, which, ("probs", "greedy", "logp", "values"), True)
    _sync(case.device)
    return {k: v.permute(1, 2, 0, *range(3, v.dim())) for k, v in res.items() if not k.startswith("h_last")}


REF_OF = (("probs_ko", "probs"), ("logp_ko", "logp"), ("values_ko", "values"), ("greedy", "greedy"), ("h_actor_ko", "h_actor"), ("h_critic_ko", "h_critic"))
BASE_OF = (("probs", "probs"), ("logp", "logp"), ("values", "values"), ("greedy_base", "greedy"))


def _assert_job_is_trace(got, q, ref, what):
    for mine, theirs in REF_OF:
        if mine in got:
            assert torch.equal(_bits(got[mine][:, :, :, q]), _bits(ref[theirs])), (what, mine, "differs from the trace of the modified copy")


def _same(a, b, what, keys=None):
    for k in (keys or sorted(set(a) & set(b))):
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def _slots(res, idx):
    return {k: v[:, :, :, idx] for k, v in res.items() if k in PAIR_KEYS}


# ------------------------------------------------------------------------------------------------ 1: the bits of a re-run
def op_call(case, jobs, win, which=2, want=OP_WANT, knock=None, baseline=None, out=None, packed="auto", **over):
    """ops.policy_knockout_trace on the case's window with the recorded start states and actions"""
    mac, nA = case.mac, case.dims[0]
    start, D, H = win
    r = mac._rows(case.batch, start, H)
    ha, hc = r.field("rnn_states_actors", torch.float32)[:, start], r.field("rnn_states_critics", torch.float32)[:, start]
    kw = dict(hidden0_actor=ha, hidden0_critic=hc, h_strides=(ha.stride(1), ha.stride(0)), avail=r.avail,
              avail_strides=(r.avail.stride(2), r.avail.stride(1)), target=r.acts, target_strides=(r.acts.stride(2), r.acts.stride(1)),
              n_actions=mac.args.n_actions, knock=knock, baseline=baseline, want=want, packed=r.packed if packed == "auto" else packed, out=out)
    kw.update(over)
    res = ops.policy_knockout_trace(mac.actor_arena, mac.critic_arena, which, r.spec, r.E, H, D, nA, jobs, **kw)
    _sync(case.device)
    return res


def _host_pairs(case, op, jobs, win, which):
    """kl, dlogp, dvalue and shift_sq as fp32 host loops over the op's own outputs, in action / unit order, every difference, product and
    sum rounded on its own; the base's log-probabilities and states are those of the first -1 job's slot"""
    start, D, H = win
    nA, E = case.dims[:2]
    b = jobs.index(-1)
    f32 = np.float32
    out = {}
    if which != 1:
        lp = op["logp_all_ko"].cpu().numpy()
        pb = op["probs"].cpu().numpy()
        av = case.f["avail_actions"][:, start:start + H].permute(2, 0, 1, 3).numpy() != 0
        kl = np.zeros(lp.shape[:4], f32)
        for a in range(lp.shape[-1]):
            d = (lp[:, :, :, b:b + 1, a] - lp[..., a]).astype(f32)
            t = (pb[..., None, a] * d).astype(f32)
            kl = np.where(av[..., None, a], (kl + t).astype(f32), kl)
        out["kl"] = kl
        out["dlogp"] = (op["logp_ko"].cpu().numpy() - op["logp"].cpu().numpy()[..., None]).astype(f32)
    if which != 0:
        out["dvalue"] = (op["values_ko"].cpu().numpy() - op["values"].cpu().numpy()[..., None]).astype(f32)
    for net in (("actor",) if which == 0 else ("critic",) if which == 1 else ("actor", "critic")):
        h = op["h_ko_" + net].cpu().numpy()
        acc = np.zeros(h.shape[:4], f32)
        for u in range(M):
            d = (h[..., u] - h[:, :, :, b:b + 1, u]).astype(f32)
            acc = (acc + (d * d).astype(f32)).astype(f32)
        out["shift_sq_" + net] = acc
    return out


def check_same_bits(device, dims, J, win, opt):
    """1: every job against the trace of an explicit copy, bit for bit; the base against the trace of the batch; kl, dlogp, dvalue and
    shift_sq against fp32 host loops over the outputs; shapes and dtypes"""
    case = _case(dims, opt, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    which = opt.get("which", "both")
    jobs = job_list(N, J)
    got = run(case, win, entities=jobs, which=which, want=ALL_WANT)
    assert got["knocked"] == tuple(jobs) and got["sources"] == case.names and got["window"] == win
    for k in PAIR_KEYS:
        on = which != ("actor" if k in ("dvalue", "values_ko", "state_shift_critic", "h_critic_ko") else "critic")
        assert (k in got) == on, (k, which)
        if on:
            assert got[k].shape[:4] == (E, H, nA, J), (k, got[k].shape)
    if which != "critic":
        assert got["greedy"].dtype == torch.int64 and got["flip"].dtype == torch.bool and got["probs_ko"].shape == (E, H, nA, J, n_act)
        assert got["h_actor_ko"].shape == (E, H, nA, J, M)
        assert torch.equal(got["target_action"].cpu(), case.f["actions"][:, start:start + H, :, 0])
    base = window_trace(case, case.f, start, H, which)
    for mine, theirs in BASE_OF:
        if mine in got:
            assert torch.equal(_bits(got[mine]), _bits(base[theirs])), (dims, win, mine, "the base chain differs from the trace")
    if start == 0:                                                           # ... and the public method on the copy sliced to the window
        sliced = copy.copy(case)
        sliced.T1 = H
        pub = case.mac.policy_trace(sliced.to_batch({k: v[:, :H] for k, v in case.f.items()}), which=which, want=("probs", "greedy", "logp", "values"),
                                    return_hidden=True)
        _sync(device)
        for mine, theirs in BASE_OF:
            if mine in got:
                assert torch.equal(_bits(got[mine]), _bits(pub[theirs])), (dims, win, mine, "the base chain differs from policy_trace")
    done = set()
    for q, j in enumerate(jobs):
        if j in done:
            continue
        done.add(j)
        ref = window_trace(case, window_fields(case, j, start, D), start, H, which)
        _assert_job_is_trace(got, q, ref, (dims, win, opt, "job", j))
    for q, j in enumerate(jobs):                                             # duplicates of a job carry the same bits
        p = jobs.index(j)
        for k in PAIR_KEYS:
            if k in got and p != q:
                assert torch.equal(_bits(got[k][:, :, :, q]), _bits(got[k][:, :, :, p])), (k, "two slots of the same job differ", p, q)
    # the differences: fp32 host loops over the op's outputs
    w = {"actor": 0, "critic": 1, "both": 2}[which]
    ojobs = jobs + [-1]
    op = op_call(case, ojobs, win, which=w)
    host = _host_pairs(case, op, ojobs, win, w)
    for k, ref in host.items():
        assert np.array_equal(op[k].cpu().numpy().view(np.int32), ref.view(np.int32)), (dims, win, opt, k, "differs from the fp32 host loop")
        name = k.replace("shift_sq", "state_shift")
        mine = got[name].permute(2, 0, 1, 3)
        theirs = torch.from_numpy(ref[..., :J]).to(mine.device)              # (the method takes torch's sqrt where the sums live)
        assert torch.equal(_bits(mine), _bits(theirs.sqrt() if k.startswith("shift") else theirs)), (dims, win, opt, name, "method != op")
    return {}


# ------------------------------------------------------------------------------------------------ 2: knockout() at h = 0
def check_agrees_with_knockout(device, dims=DIMS, win=WIN):
    """2: at h = 0 kl, dlogp and dvalue agree with knockout(steps=start) from the same start state within 1e-5"""
    case = get_case(dims, device)
    start, D, H = win
    got = run(case, win)
    ha, hc = case.f["rnn_states_actors"][:, start:start + 1].to(device), case.f["rnn_states_critics"][:, start:start + 1].to(device)
    one = case.mac.knockout(case.batch, steps=slice(start, start + 1), hidden=(ha, hc))
    _sync(device)
    worst = {}
    for k in ("kl", "dlogp", "dvalue"):
        diff = (got[k][:, 0] - one[k][:, 0]).abs().max().item()
        print("knockout_trace vs knockout at h = 0:", k, diff)
        _worse(worst, k + "_vs_knockout", diff)
        assert diff <= TOL, (k, diff)
    assert bool((got["kl"][:, 0] > 0).any())
    return worst


# ------------------------------------------------------------------------------------------------ 3: fp64
def _oracle_chain(case, f, start, H, dtype):
    h0a, h0c = f["rnn_states_actors"][:, start], f["rnn_states_critics"][:, start]
    return _method_reference(case.mac, f, dtype, h0a, h0c, start, H)        # [nA, E, H, ..]


def check_vs_fp64(device, dims, J, win, opt):
    """3: every float output against the fp64 oracle chain on the modified inputs under the rule; greedy and flip away from fp64 ties"""
    case = _case(dims, opt, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    which = opt.get("which", "both")
    jobs = job_list(N, J)
    got = run(case, win, entities=jobs, which=which, want=ALL_WANT)
    av = case.f["avail_actions"][:, start:start + H].permute(2, 0, 1, 3) != 0                   # [nA, E, H, n_act]
    has = av.any(-1)
    tgt = case.f["actions"][:, start:start + H, :, 0].permute(2, 0, 1).unsqueeze(-1)          # [nA, E, H, 1]
    refs = {}
    for dt in (torch.float64, torch.float32):
        base = _oracle_chain(case, case.f, start, H, dt)
        cache = {}
        for j in set(jobs):
            cache[j] = base if j < 0 else _oracle_chain(case, window_fields(case, j, start, D), start, H, dt)
        st = lambda k: torch.stack([cache[j][k] for j in jobs], 3)                              # noqa: E731  [nA, E, H, J, ..]
        lb = base["probs"].clamp_min(1e-300 if dt == torch.float64 else 1e-38).log()
        lk = st("probs").clamp_min(1e-300 if dt == torch.float64 else 1e-38).log()
        r = dict(probs_ko=st("probs"), values_ko=st("values"), h_actor_ko=st("h_actor"), h_critic_ko=st("h_critic"))
        r["logp_full"] = lk.gather(-1, tgt.unsqueeze(3).expand(-1, -1, -1, J, -1))[..., 0]
        r["dlogp"] = r["logp_full"] - lb.gather(-1, tgt)[..., 0].unsqueeze(-1)
        r["kl"] = torch.where(av.unsqueeze(3), base["probs"].unsqueeze(3) * (lb.unsqueeze(3) - lk), torch.zeros_like(lk)).sum(-1)
        r["dvalue"] = r["values_ko"] - base["values"].unsqueeze(-1)
        r["state_shift_actor"] = (r["h_actor_ko"] - base["h_actor"].unsqueeze(3)).norm(dim=-1)
        r["state_shift_critic"] = (r["h_critic_ko"] - base["h_critic"].unsqueeze(3)).norm(dim=-1)
        r["base"] = base
        refs[dt] = r
    r64, r32 = refs[torch.float64], refs[torch.float32]
    worst = {}
    skipped = total = 0
    keys = [k for k in ("probs_ko", "logp_ko", "values_ko", "h_actor_ko", "h_critic_ko", "kl", "dlogp", "dvalue", "state_shift_actor", "state_shift_critic")
            if k in got]
    for i in range(nA):
        for key in keys:
            g = got[key][:, :, i].cpu()                                       # [E, H, J, ..]
            ref, ref32 = (r["logp_full" if key == "logp_ko" else key][i] for r in (r64, r32))
            if key in ("logp_ko", "dlogp"):                                   # (a row with no available action: fp32 gives 0, fp64 -log n)
                g, ref, ref32 = g[has[i]], ref[has[i]], ref32[has[i]]
            err, e32 = _rel(g, ref), _rel(ref32, ref)
            bound = max(TOL, E32_FACTOR * e32)
            print((dims, win, opt), "agent", i, key, "err", err, "e32", e32, "bound", bound)
            _worse(worst, key, err)
            _worse(worst, key + "_e32", e32)
            assert err <= bound, (dims, win, opt, i, key, err, e32)
        if which != "critic":
            knocked = torch.zeros(H, dtype=torch.bool)
            knocked[:D] = True
            changed = (torch.tensor([j >= 0 for j in jobs])[None, None, :] & (av[i].sum(-1) >= 2)[:, :, None]) & knocked[None, :, None]
            if n_act > 1 and bool(changed.any()):                             # (E = 1, D = 1 at step 0 knocks the one-action row only)
                assert bool((r64["kl"][i][changed] > KL_FLOOR).any()), (dims, win, i, "no knocked pair has fp64 KL > 1e-6")
            p64, b64 = r64["probs_ko"][i], r64["base"]["probs"][i]
            top, topb = p64.topk(min(2, n_act), -1).values, b64.topk(min(2, n_act), -1).values
            clear = (top[..., 0] - top[..., -1] >= GAP) if n_act > 1 else torch.ones(E, H, J, dtype=torch.bool)
            clear_b = (topb[..., 0] - topb[..., -1] >= GAP) if n_act > 1 else torch.ones(E, H, dtype=torch.bool)
            same = got["greedy"][:, :, i].cpu() == p64.argmax(-1)
            assert bool((same | ~clear).all()), (dims, win, i, "greedy differs from the fp64 argmax away from a tie")
            flip64 = p64.argmax(-1) != b64.argmax(-1).unsqueeze(-1)
            both = clear & clear_b.unsqueeze(-1)
            assert bool(((got["flip"][:, :, i].cpu() == flip64) | ~both).all()), (dims, win, i, "flip differs from fp64 away from a tie")
            skipped += int((~both & has[i][:, :, None]).sum())
            total += int(has[i].sum()) * J
    if which != "critic":
        worst["greedy_skipped_share"] = skipped / max(total, 1)
        assert skipped <= SKIP_CAP * total, (dims, win, "too many rows at an fp64 tie", skipped, total)
    return worst


# ------------------------------------------------------------------------------------------------ 4: exact zeros
def check_exact_zeros(device, dims, win, opt, mode):
    """4: a job -1, an entity whose columns are already zero over the knocked steps and a baseline equal to the entity's own row give
    kl = dlogp = dvalue = state_shift = 0.0 exactly at every one of the H steps, and the base chain's bits"""
    case = _case(dims, opt, device)
    N = dims[3]
    start, D, H = win
    base = _baseline(case, 9) if mode == "baseline" else None
    f = window_fields(case, 1, start, D, None, base)
    jobs = [1, 0, -1, 1] + job_list(N, 13)                                    # 17 slots: the unchanged job in both tiles
    got = run(case, win, batch=case.to_batch(f), entities=jobs, baseline=base, want=ALL_WANT)
    for q, j in enumerate(jobs):
        if j not in (1, -1):
            continue
        for k in ("kl", "dlogp", "dvalue", "state_shift_actor", "state_shift_critic"):
            assert got[k].shape[1] == H and bool((got[k][:, :, :, q] == 0).all()), (mode, k, "is not exactly 0 on an unchanged job", q, j)
        for mine, theirs in (("probs_ko", "probs"), ("logp_ko", "logp"), ("values_ko", "values"), ("greedy", "greedy_base")):
            assert torch.equal(_bits(got[mine][:, :, :, q]), _bits(got[theirs])), (mode, mine, "differs from the base", q, j)
        assert not bool(got["flip"][:, :, :, q].any())
    for k in ("dvalue", "kl", "state_shift_actor", "state_shift_critic"):
        assert bool((got[k][:, :, :, 1] != 0).any()), (k, "the changed job moved nothing")
    if H > D:
        assert bool((got["state_shift_critic"][:, D:, :, 1] != 0).all()), "the knock leaves no echo in the state"
    return {}


# ------------------------------------------------------------------------------------------------ 5: echo semantics
def check_echo(device, dims=DIMS):
    """5: with D = 1, H = 3 the steps 1 .. 2 of job j are the plain trace of the UNMODIFIED batch from the job's state after step 0;
    D = H equals that many chained one-step re-runs on the modified copy"""
    case = get_case(dims, device)
    nA, E, S, N = dims[:4]
    start = 1
    got = run(case, (start, 1, 3), want=ALL_WANT)
    for j in range(N):
        h0 = (got["h_actor_ko"][:, 0, :, j].contiguous(), got["h_critic_ko"][:, 0, :, j].contiguous())
        ref = window_trace(case, case.f, start + 1, 2, hidden0=h0)
        for mine, theirs in REF_OF:
            assert torch.equal(_bits(got[mine][:, 1:, :, j]), _bits(ref[theirs])), (j, mine, "the echo steps do not see the recorded inputs")
    assert bool((got["kl"][:, 1:] != 0).any()), "no echo at all"
    full = run(case, (start, 3, 3), want=ALL_WANT)
    for j in range(N):
        f = window_fields(case, j, start, 3)
        h0 = None
        for h in range(3):
            ref = window_trace(case, f, start + h, 1, hidden0=h0)
            for mine, theirs in REF_OF:
                assert torch.equal(_bits(full[mine][:, h:h + 1, :, j]), _bits(ref[theirs])), (j, h, mine, "D = H differs from chained one-step re-runs")
            h0 = (ref["h_actor"][:, 0].contiguous(), ref["h_critic"][:, 0].contiguous())
    return {}


# ------------------------------------------------------------------------------------------------ 6: independence, repeatability
def _pair_bytes(nA, H, n_act):
    return nA * H * (4 * 5 + 8 + 4 * (2 + n_act) + 8 * M)


def check_independence(device, reps=2, dims=(1, 2, 4, 7, 5, 5), win=(1, 2, 3)):
    """6: a slot's bits do not change under permuted, duplicated or subsetted jobs, J or E split by a tiny max_workspace_mb, a shorter H
    (a prefix), packed or in-place fc1 operands, or the outputs asked for; each ``reps`` times"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    want = ALL_WANT + ("summary",)
    full = run(case, win, want=want)
    gen = torch.Generator().manual_seed(2)
    perm = torch.randperm(N, generator=gen).tolist()
    for _ in range(reps):
        _same(run(case, win, want=want), full, "repeat")
        for jobs in (perm, [3, 3, 6, 3, -1, 0] * 6, [4]):
            part = run(case, win, entities=jobs, want=ALL_WANT)
            idx = [j for j in jobs if j >= 0]
            pos = [q for q, j in enumerate(jobs) if j >= 0]
            _same(_slots(part, pos), _slots(full, idx), ("jobs", jobs))
            _same(part, full, ("base with jobs", jobs), BASE_KEYS)
        gi = 4 * L.AC_TRACE_GI
        env = 2 * nA * H * gi
        job = _pair_bytes(nA, H, n_act) + 2 * nA * D * gi * 16 // 15 + 1
        for mb in ((E * env + 3 * E * job) / 2 ** 20, (env + N * job) / 2 ** 20, 1e-9):            # J split; E split; one pair per launch
            _same(run(case, win, want=want, max_workspace_mb=mb), full, ("max_workspace_mb", mb))
        for h in range(D, H):
            short = run(case, (start, D, h), want=ALL_WANT)
            _same(short, {k: (v[:, :h] if torch.is_tensor(v) else v) for k, v in full.items()}, ("horizon", h), PAIR_KEYS + BASE_KEYS)
        keep = os.environ.get("IPLAN_NO_FC1_PACK")
        os.environ["IPLAN_NO_FC1_PACK"] = "1"                                # Fc1Pack.get returns None: the arena is read in place
        try:
            assert case.mac.fc1_pack.get(None) is None
            inplace = run(case, win, want=want)
        finally:
            if keep is None:
                del os.environ["IPLAN_NO_FC1_PACK"]
            else:
                os.environ["IPLAN_NO_FC1_PACK"] = keep
        _same(inplace, full, "packed != in place")
        for w in ((), ("probs_ko",), ("values_ko", "summary"), ("h_critic_ko",)):
            _same(run(case, win, want=w), full, ("want", w))
        for which in ("actor", "critic"):
            _same(run(case, win, which=which, want=ALL_WANT), full, ("which", which))
    op_full = op_call(case, list(range(N)), win)
    for w in (("kl",), ("dvalue",), ("base",), ("shift_sq",), ("greedy_ko", "probs_ko"), ("logp_ko", "values_ko", "dlogp", "h_ko")):
        _same(op_call(case, list(range(N)), win, want=w), op_full, ("op want", w))
    return {}


# ------------------------------------------------------------------------------------------------ 7: ownership (the op)
def _op_shapes(case, J, win):
    nA, E, S, N, d, n_act = case.dims
    start, D, H = win
    pair = (nA, E, H, J)
    row = (nA, E, H)
    return dict(logp=row, values=row, target_action=row, greedy=row, probs=row + (n_act,), kl=pair, dlogp=pair, dvalue=pair, greedy_ko=pair,
                probs_ko=pair + (n_act,), logp_ko=pair, values_ko=pair, shift_sq_actor=pair, shift_sq_critic=pair, h_ko_actor=pair + (M,),
                h_ko_critic=pair + (M,), logp_all_ko=pair + (n_act,))


def _sentinels(shapes, device, shift=0.0):
    """every output a 16-byte aligned view inside a sentinel-filled buffer whose first and last four elements are NaN (floats)"""
    bufs = {}
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        if k in ("target_action", "greedy", "greedy_ko"):
            sent = torch.arange(n + 64, dtype=torch.int64) * 7 + 1000
        else:
            sent = 0.5 + shift + (torch.arange(n + 64, dtype=torch.float32) % 1021) / 1024.0
            sent[:4] = float("nan")
            sent[-4:] = float("nan")
        buf = sent.clone().to(device)
        bufs[k] = (sent, buf, buf[32:32 + n].view(shape))
    return bufs


OWNED = dict(base=("logp", "values", "target_action", "greedy", "probs"), shift_sq=("shift_sq_actor", "shift_sq_critic"), h_ko=("h_ko_actor", "h_ko_critic"))
ACTOR_KEYS = ("logp", "target_action", "greedy", "probs", "kl", "dlogp", "greedy_ko", "probs_ko", "logp_ko", "shift_sq_actor", "h_ko_actor", "logp_all_ko")


def check_ownership(device, dims, J, win):
    """7: outputs carved out of sentinel-filled, NaN-edged buffers keep their surroundings, every owned element is written, outputs not
    asked for stay untouched; the gi_ko workspace of the call, pre-filled with NaN, holds no NaN in the slots of real columns afterwards"""
    case = get_case(dims, device)
    nA, E, S, N = dims[:4]
    start, D, H = win
    jobs = job_list(N, J)
    base = [b.to(device) for b in _baseline(case).values()]
    shapes = _op_shapes(case, J, win)
    ref = op_call(case, jobs, win, baseline=base)
    assert set(ref) == set(shapes)
    for which, want in ((2, OP_WANT), (2, ("kl",)), (0, ("base", "probs_ko", "h_ko")), (1, ("dvalue", "values_ko", "shift_sq")),
                        (2, ("greedy_ko", "dlogp", "logp_ko"))):
        bufs = _sentinels(shapes, device)
        got = op_call(case, jobs, win, which=which, want=want, baseline=base, out={k: v[2] for k, v in bufs.items()})
        owned = {k for w in want for k in OWNED.get(w, (w,)) if (k in ACTOR_KEYS and which != 1) or (k not in ACTOR_KEYS and which != 0)}
        assert set(got) == owned, (which, want, sorted(got), sorted(owned))
        for k, (sent, buf, view) in bufs.items():
            host = buf.cpu()
            if k not in owned:
                assert torch.equal(_bits(host), _bits(sent)), (dims, which, want, k, "was not asked for and was written")
                continue
            assert torch.equal(_bits(view), _bits(ref[k])), (dims, k, "differs inside a sentinel buffer")
            n = view.numel()
            assert torch.equal(_bits(host[:32]), _bits(sent[:32])) and torch.equal(_bits(host[32 + n:]), _bits(sent[32 + n:])), \
                (dims, k, "an element outside the owned region was written")
    b2 = _sentinels(shapes, device, 0.25)                                     # every owned element is written
    JT = (J + 14) // 15
    gi = torch.full((2, nA, E, D, JT, 16, L.AC_TRACE_GI), float("nan"), device=device)
    out = {k: v[2] for k, v in b2.items()}
    out["gi_ko"] = gi
    op_call(case, jobs, win, baseline=base, want=OP_WANT + ("gi_ko",), out=out)
    for k in shapes:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (dims, k, "an owned element was left unwritten")
    gi = gi.cpu()
    for jt in range(JT):
        real = [n for n in range(15) if 15 * jt + n < J] + [15]
        assert not bool(torch.isnan(gi[:, :, :, :, jt, real]).any()), ("gi_ko has a NaN in an owned slot", jt)
        rest = [n for n in range(15) if 15 * jt + n >= J]
        assert bool(torch.isnan(gi[:, :, :, :, jt, rest]).all()), ("gi_ko was written outside the owned slots", jt)
    return {}


# ------------------------------------------------------------------------------------------------ 8: touches nothing
def check_touches_nothing(device, reps=1):
    """8: parameters, both arenas' gradient entries, the optimisers' state, hidden_states, the batch and the generator states are
    bit-identical before and after knockout_trace(); a train() after it gives the bits of one without it"""
    results = []
    for with_call in (False, True):
        args, mac, learner, batch = SC._learner(device)
        torch.manual_seed(83)
        if with_call:
            for arena in (mac.actor_arena, mac.critic_arena):
                arena.grad.fill_(0.7071)
            watched = [t for t in SC._state_tensors(learner) if t.device.type == torch.device(device).type]
            assert any(t.data_ptr() == mac.actor_arena.data.data_ptr() for t in watched) and len(watched) > 8, len(watched)
            before = [t.clone() for t in watched]
            fields = {k: v.clone() for k, v in batch.data.items()}
            states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, np.random.get_state()[1].copy())
            mac.hidden_states = "untouched"
            first = None
            for _ in range(reps):
                res = mac.knockout_trace(batch, start=1, duration=1, horizon=3, want=ALL_WANT + ("summary",),
                                         baseline={"history": torch.ones(args.obs_shape_single)})
                _sync(device)
                if first is not None:
                    _same(res, first, "repeat")
                first = res
            assert torch.isfinite(res["kl"]).all() and torch.isfinite(res["dvalue"]).all() and res["dvalue"].abs().sum() > 0
            assert torch.equal(torch.get_rng_state(), states[0]) and np.array_equal(np.random.get_state()[1], states[2])
            if states[1] is not None:
                assert torch.equal(torch.cuda.get_rng_state(), states[1])
            assert mac.hidden_states == "untouched"
            mac.hidden_states = None
            for t, b in zip(watched, before):
                assert torch.equal(_bits(t), _bits(b)), ("a tensor of the learner changed", tuple(t.shape))
            for arena in (mac.actor_arena, mac.critic_arena):
                assert torch.equal(arena.grad, torch.full_like(arena.grad, 0.7071)), "a gradient entry was written"
                arena.grad.zero_()
            for k, v in fields.items():
                assert torch.equal(batch.data[k], v), (k, "the batch was written")
        else:
            for arena in (mac.actor_arena, mac.critic_arena):
                arena.grad.zero_()
        learner.train(0)
        _sync(device)
        results.append((mac.actor_arena.data.clone(), mac.critic_arena.data.clone()))
    (a0, c0), (a1, c1) = results
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    return {}


# ------------------------------------------------------------------------------------------------ 9: the method
def _host_summary(case, res, jobs, win, presence_col=0):
    """the float64 host loop: means over the environments with weight filled[:, start + h], over the pairs whose entity is present in at
    least one knocked step"""
    nA, E = case.dims[:2]
    start, D, H = win
    hist = case.f["history"]
    filled = case.f["filled"].reshape(E, -1).double()
    shift = res["state_shift_actor"]
    cols = dict(echo_kl=res["kl"].double(), echo_abs_dvalue=res["dvalue"].double().abs(), echo_flip_rate=res["flip"].double(), echo_state_shift=shift.double())
    out = {k: np.zeros((nA, H, len(jobs))) for k in cols}
    for i in range(nA):
        for q, j in enumerate(jobs):
            for h in range(H):
                num, den = {k: 0.0 for k in cols}, 0.0
                for e in range(E):
                    if j >= 0 and presence_col >= 0 and not bool((hist[e, start:start + D, i, j, presence_col] != 0).any()):
                        continue
                    wt = float(filled[e, start + h])
                    den += wt
                    for k, v in cols.items():
                        num[k] += wt * float(v[e, h, i, q])
                for k in cols:
                    out[k][i, h, q] = num[k] / den if den > 0 else 0.0
    return out


def check_methods(device, tmp_path):
    """9: on a loaded checkpoint, numpy and device inputs agree; the summary against a float64 host loop; target="greedy" and the
    hidden0 forms"""
    dims, win = (2, 3, 4, 3, 5, 5), (1, 2, 3)
    start, D, H = win
    src = get_case(dims, device)
    case = copy.copy(src)
    case.mac = make_mac(src.args, 77)
    src.mac.save_models(str(tmp_path))
    assert not torch.equal(case.mac.actor_arena.data, src.mac.actor_arena.data)
    case.mac.load_models([str(tmp_path)])
    nA, E, S, N = dims[:4]
    jobs = [2, -1, 0, 1, 2]
    from iplan_amd import synth
    np_batch = synth.DictBatch({k: v.numpy() for k, v in case.f.items()}, E, case.T1)
    want = ALL_WANT + ("summary",)
    r_dev = run(case, win, entities=jobs, want=want)
    r_np = run(case, win, batch=np_batch, entities=jobs, want=want)
    _same(r_dev, run(src, win, entities=jobs, want=want), "the loaded checkpoint differs from its source")
    for k, v in r_dev.items():
        if k in ("knocked", "sources", "window"):
            assert r_np[k] == v
            continue
        assert isinstance(r_np[k], np.ndarray) and torch.is_tensor(v) and v.device.type == torch.device(device).type, k
        assert np.array_equal(r_np[k], v.cpu().numpy()), (k, "numpy-backed and device-backed batches differ")
    # horizon=None: up to the last step; duration=None: throughout
    rest = case.mac.knockout_trace(case.batch, entities=jobs, start=start, duration=None)
    assert rest["window"] == (start, case.T1 - start, case.T1 - start) and rest["kl"].shape == (E, case.T1 - start, nA, len(jobs))
    # the summary
    cpu = {k: v.cpu() for k, v in r_dev.items() if torch.is_tensor(v)}
    worst = {}
    for pc in (0, -1):
        got = r_dev if pc == 0 else run(case, win, entities=jobs, want=("summary",), presence_col=-1)
        host = _host_summary(case, cpu, jobs, win, presence_col=pc)
        for k, ref in host.items():
            assert got[k].dtype == torch.float64 and got[k].shape == (nA, H, len(jobs))
            err = np.abs(got[k].cpu().numpy() - ref).max()
            _worse(worst, k + ("" if pc == 0 else "_every_pair"), err)
            assert err <= 1e-12 * max(1.0, np.abs(ref).max()), (k, pc, err)
        assert (host["echo_kl"] > 0).any() and (host["echo_state_shift"][:, D:] > 0).any()
    # target="greedy": a* is the base chain's argmax, the same for every job; a tensor target
    gr = run(case, win, entities=jobs, target="greedy", want=("logp_ko", "probs_ko"))
    assert torch.equal(gr["target_action"], gr["greedy_base"]) and torch.equal(gr["greedy_base"], r_dev["greedy_base"])
    pick = gr["probs_ko"].clamp_min(1e-38).log().gather(-1, gr["target_action"][:, :, :, None, None].expand(-1, -1, -1, len(jobs), -1))[..., 0]
    has = (case.f["avail_actions"][:, start:start + H].sum(-1) > 0).to(pick.device)
    assert float((pick - gr["logp_ko"])[has].abs().max()) <= 1e-5
    as_t = run(case, win, entities=jobs, target=gr["target_action"], want=("logp_ko",))
    _same(as_t, gr, "a tensor target differs from the same actions by name", ("logp_ko", "dlogp", "kl", "logp", "target_action"))
    # hidden0: the recorded states given explicitly; zeros
    ha, hc = case.f["rnn_states_actors"][:, start].to(device), case.f["rnn_states_critics"][:, start].to(device)
    _same(run(case, win, entities=jobs, hidden0=(ha, hc), want=want), r_dev, "hidden0 given != hidden0 recorded")
    z = run(case, win, entities=jobs, hidden0="zeros", want=ALL_WANT)
    _same(z, run(case, win, entities=jobs, hidden0=(torch.zeros_like(ha), torch.zeros_like(hc)), want=ALL_WANT), 'hidden0="zeros" != zero tensors')
    assert not torch.equal(z["values_ko"], r_dev["values_ko"])
    zt = window_trace(case, window_fields(case, 2, start, D), start, H, hidden0="zeros")
    _assert_job_is_trace(z, 0, zt, 'hidden0="zeros"')
    return worst


def check_method_refusals(device, dims=DIMS):
    """9: ValueError before anything is launched; layer_N / recurrent_N other than 1 raise NotImplementedError"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    mac, T1 = case.mac, case.T1

    def refuses(exc=ValueError, **kw):
        try:
            mac.knockout_trace(case.batch, **kw)
        except exc:
            return
        raise AssertionError(f"knockout_trace accepted {kw}")
    refuses(start=-1)
    refuses(start=T1)
    refuses(start=0.5)
    refuses(start=1, horizon=T1)
    refuses(horizon=0)
    refuses(horizon=T1 + 1)
    refuses(horizon=1.5)
    refuses(duration=0)
    refuses(duration=3, horizon=2)
    refuses(start=T1 - 1, duration=2)
    refuses(entities=[])
    refuses(entities=[N])
    refuses(entities=[-2])
    refuses(sources=())
    refuses(sources=("history", "intent"))
    refuses(baseline={"intent": torch.zeros(3)})
    refuses(baseline=torch.zeros(d))
    refuses(baseline={"history": torch.zeros(d + 1)})
    refuses(want=("kl", "entity"))
    refuses(which="all")
    refuses(target="sampled")
    refuses(hidden0="ones")
    refuses(presence_col=d)
    refuses(max_workspace_mb=0)
    no_gat = get_case((1, 2, 4, 3, 5, 5), device, (("gat", False),))
    for kw in (dict(sources=("attention_latent",)), dict(baseline={"attention_latent": torch.zeros(32)})):
        try:
            no_gat.mac.knockout_trace(no_gat.batch, **kw)                    # an absent source
        except ValueError:
            continue
        raise AssertionError(f"knockout_trace accepted {sorted(kw)} without a GAT")
    ok = mac.knockout_trace(case.batch, entities=[1])
    assert ok["kl"].shape == (E, T1, nA, 1) and ok["window"] == (0, 1, T1)
    orig = mac.args
    try:
        mac.args = copy.copy(orig)
        mac.args.layer_N = 2
        refuses(NotImplementedError)
        mac.args.layer_N, mac.args.recurrent_N = 1, 2
        refuses(NotImplementedError)
    finally:
        mac.args = orig
    return {}


def _code(name):
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iplan_hip.h")).read()
    return int(re.search(name + r"\s*=\s*(-?\d+)", text).group(1))


def check_bad_arguments(device, dims=DIMS, win=WIN):
    """9 (the entry point): each invalid descriptor is refused by the host-side check with IPLAN_EINVAL / IPLAN_EALIGN and a message;
    nothing is launched, so the sentinel-filled outputs stay as they were"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    mac = case.mac
    jobs = [0, 2, -1]
    good = op_call(case, jobs, win)
    bufs = _sentinels(_op_shapes(case, len(jobs), win), device)
    r = mac._rows(case.batch, start, H)
    ha, hc = r.field("rnn_states_actors", torch.float32)[:, start], r.field("rnn_states_critics", torch.float32)[:, start]
    lib = ops._lib(None)
    EINVAL = _codes()
    EALIGN = _code("IPLAN_EALIGN")
    fn = lib.c.iplan_ac_knockout_trace
    # a descriptor of the call that was just made: built by hand from the op's pieces, launched never
    a = L.AcKnockoutTraceArgs()
    ops._ac_rows(a.base, mac.actor_arena, mac.critic_arena, 2, r.spec, E, H, nA)
    ops._fill_acnet(a.base.actor, mac.actor_arena, L.ACTOR_PARAM_ORDER, n_act)
    ops._fill_acnet(a.base.critic, mac.critic_arena, L.CRITIC_PARAM_ORDER, 1)
    a.base.hidden0_actor, a.base.hidden0_critic = ha.data_ptr(), hc.data_ptr()
    a.base.h0_s_net, a.base.h0_s_chain = ha.stride(1), ha.stride(0)
    gi = torch.zeros(2 * nA * E * H * L.AC_TRACE_GI + 4, device=device)
    gi_ko = torch.zeros(2 * nA * E * D * 16 * L.AC_TRACE_GI + 4, device=device)
    a.base.gi, a.gi_ko = gi.data_ptr(), gi_ko.data_ptr()
    a.D, a.J = D, len(jobs)
    j_host = (L.C.c_int32 * 3)(*jobs)
    j_dev = torch.tensor(jobs, dtype=torch.int32, device=device)
    a.jobs, a.jobs_host = j_dev.data_ptr(), L.C.cast(j_host, L.C.c_void_p)
    for k in range(3):
        a.knock[k] = 1
    a.kl, a.dvalue = bufs["kl"][2].data_ptr(), bufs["dvalue"][2].data_ptr()
    a.h_ko_actor = bufs["h_ko_actor"][2].data_ptr()

    def refused(args_ref, code=EINVAL, **fields):
        keep_f = {}
        for k, v in fields.items():
            obj, name = a, k
            while "." in name:
                head, name = name.split(".", 1)
                obj = getattr(obj, head)
            if "[" in name:
                name, idx = name[:-1].split("[")
                arr = getattr(obj, name)
                keep_f[k] = (arr, int(idx), arr[int(idx)])
                arr[int(idx)] = v
            else:
                keep_f[k] = (obj, name, getattr(obj, name))
                setattr(obj, name, v)
        rc = fn(args_ref, L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for obj, name, v in keep_f.values():
            if isinstance(name, int):
                obj[name] = v
            else:
                setattr(obj, name, v)
        assert rc == code and rc < 0 and "iplan_ac_knockout_trace" in msg, (fields, rc, msg)
        return msg

    refused(None)
    ref = L.C.byref(a)
    refused(ref, **{"base.which": 3})
    refused(ref, **{"base.n_agents": 0})
    refused(ref, **{"base.E": 0})
    refused(ref, **{"base.S": 0})
    assert "D=" in refused(ref, D=0)
    assert "D=" in refused(ref, D=H + 1)
    assert "phases" in refused(ref, **{"base.phases": 3})
    refused(ref, **{"base.feat.N": 65})
    refused(ref, **{"base.feat.T": H + 1})
    refused(ref, **{"base.feat.T_phys": H - 1})
    refused(ref, **{"base.feat.n_id": -1})
    assert "source 0" in refused(ref, **{"base.feat.src[0]": None})
    refused(ref, J=0)
    refused(ref, jobs=None)
    refused(ref, jobs_host=None)
    bad = (L.C.c_int32 * 3)(0, N, -1)
    assert "job 1" in refused(ref, jobs_host=L.C.cast(bad, L.C.c_void_p))
    bad2 = (L.C.c_int32 * 3)(0, 1, -2)
    assert "job 2" in refused(ref, jobs_host=L.C.cast(bad2, L.C.c_void_p))
    assert "too many" in refused(ref, **{"base.E": 2 ** 27})
    assert "absent" in refused(ref, **{"base.feat.w[2]": 0})
    assert "absent" in refused(ref, **{"base.feat.w[2]": 0, "knock[2]": 0, "baseline[2]": 64})
    assert "base's outputs" in refused(ref, **{"base.entropy": 64})
    assert "base's outputs" in refused(ref, **{"base.h_last_actor": 64})
    assert "base's outputs" in refused(ref, **{"base.h_all_critic": 64})
    refused(ref, **{"base.actor.n_out": 17})
    refused(ref, **{"base.actor.params": None})
    refused(ref, **{"base.critic.n_out": 2})
    refused(ref, **{"base.critic.params": None})
    assert "no output" in refused(ref, kl=None, dvalue=None, h_ko_actor=None)
    assert "no output" in refused(ref, kl=None, h_ko_actor=None, **{"base.which": 0})
    assert "gi_ko" in refused(ref, gi_ko=None)
    assert "echo" in refused(ref, **{"base.gi": None})
    for field, v in (("gi_ko", gi_ko.data_ptr() + 4), ("base.gi", gi.data_ptr() + 4), ("h_ko_actor", a.h_ko_actor + 4), ("h_ko_critic", 68),
                     ("base.packed_actor", 68), ("base.packed_critic", 72)):
        assert "aligned" in refused(ref, code=EALIGN, **{field: v}), field
    assert "aligned" in refused(ref, code=EALIGN, **{"base.packed_s_net": 2})

    def raises(**kw):
        try:
            op_call(case, kw.pop("jobs", jobs), kw.pop("win", win), out={k: v[2] for k, v in bufs.items()}, **kw)
        except AssertionError:
            return
        raise AssertionError(f"ops.policy_knockout_trace accepted {sorted(kw)}")
    raises(jobs=[])
    raises(jobs=[N])
    raises(jobs=[-2])
    dv = lambda t: t.to(device)                                                    # noqa: E731
    raises(baseline=[dv(torch.zeros(d + 1)), None, None])
    raises(baseline=[dv(torch.zeros(d, dtype=torch.float64)), None, None])
    raises(baseline=[None, None, None, dv(torch.zeros(4))])
    raises(knock=[True, True, True, True])
    raises(want=("kl", "entity"))
    raises(want=())
    raises(which=1, want=("kl",))
    raises(target=case.f["actions"][:, start:start + H, :, 0].to(device).int())
    raises(hidden0_actor=ha.double())
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(_bits(buf.cpu()), _bits(sent)), (k, "a refused call wrote an output")
    _same(op_call(case, jobs, win), good, "after the refusals")
    return {}


def check_abi():
    """9: the size registry of the active library knows the new struct, the ctypes mirror has its size, the entry is exported"""
    lib = ops._lib(None)
    assert "IplanAcKnockoutTraceArgs" in L.STRUCT_MIRRORS and "iplan_ac_knockout_trace" in L.ENTRY_POINTS
    n = lib.c.iplan_sizeof(b"IplanAcKnockoutTraceArgs")
    assert n > 0 and n == L.C.sizeof(L.STRUCT_MIRRORS["IplanAcKnockoutTraceArgs"]), (n, L.C.sizeof(L.STRUCT_MIRRORS["IplanAcKnockoutTraceArgs"]))
    assert hasattr(lib.c, "iplan_ac_knockout_trace")
    return {}
