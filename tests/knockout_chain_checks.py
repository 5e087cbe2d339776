"""TEST INFRASTRUCTURE: the social knock-out chain through time (csrc/policy_knockout_chain.hip, ops.policy_knockout_trace(override=,
override_base=), DcntrlMAC.knockout_trace(override=, override_base=, social=)) on whatever library is active -- the host emulator in
tests/test_emu_knockout_chain.py, the gfx950 build in tests/test_gpu_knockout_chain.py.

Cases are (nA, E, S, N, d, n_actions), J, (start, D, H) on policy_knockout_checks.Case, with two dicts: the case's options (tanh, gat,
beh, which) and the chain's (``keys``: the overridden sources; ``sources``: what the call asks to knock; ``base``: whether a base
override is given, and for which sources; ``view``: how the override lies in memory; ``inplace``: fc1 read from the arena).
Ground truth 1 (bits): job slot q against ``DcntrlMAC._trace`` on an explicit copy of the batch whose overridden fields hold
override[..., q, :, :] over the whole window and whose knocked sources have the job's entity replaced in steps start .. start + D - 1;
the base against ``_trace`` on the copy with ``override_base`` written in.
Ground truth 2 (fp64): policy_trace_checks._method_reference on the same copies, knockout_trace_checks.check_vs_fp64's rule unchanged:
error = max|got - ref64| / max(1, max|ref64|) per agent and tensor, bound = max(1e-5, E32_FACTOR x the fp32 oracle's own distance)."""
import copy
import os

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from tests import knockout_trace_checks as KT
from tests import saliency_checks as SC
from tests.oracle_checks import E32_FACTOR, _rel
from tests.policy_knockout_checks import GAP, KL_FLOOR, SKIP_CAP, _case, get_case, job_list
from tests.policy_trace_checks import _bits, _codes, _sync, _worse, make_mac

TOL = KT.TOL
M = KT.M
ALL_WANT, PAIR_KEYS, BASE_KEYS, OP_WANT = KT.ALL_WANT, KT.PAIR_KEYS, KT.BASE_KEYS, KT.OP_WANT
AL = "attention_latent"

BIT_CASES = [
    ((1, 1, 1, 2, 5, 5), 1, (0, 1, 1), {}, {}),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), {}, {}),
    ((2, 2, 4, 3, 5, 5), 4, (0, 4, 4), {}, {}),
    ((1, 1, 4, 3, 5, 5), 3, (3, 1, 1), {}, {}),
    ((1, 2, 3, 17, 5, 5), 15, (0, 2, 3), {}, {}),
    ((1, 2, 3, 17, 5, 5), 16, (0, 2, 3), {}, {}),
    ((1, 2, 3, 17, 5, 5), 17, (0, 2, 3), {}, {}),
    ((1, 2, 3, 17, 5, 5), 33, (0, 2, 3), {}, {}),
    ((5, 1, 3, 3, 5, 5), 4, (0, 1, 3), {}, {}),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), dict(which="actor"), {}),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), dict(which="critic"), {}),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), dict(tanh=True), {}),
    ((1, 2, 4, 3, 5, 5), 4, (1, 2, 3), dict(beh=False), {}),
    ((2, 2, 4, 3, 5, 5), 5, (1, 2, 3), {}, dict(keys=(AL, "history"))),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), {}, dict(sources=(AL,))),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), {}, dict(view="strided")),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), {}, dict(view="expand")),
    ((2, 2, 4, 3, 5, 5), 4, (1, 1, 3), {}, dict(inplace=True)),
    ((2, 2, 4, 3, 5, 5), 4, (1, 2, 3), {}, dict(base=())),
    ((2, 2, 4, 3, 5, 5), 5, (1, 2, 3), {}, dict(base=(AL, "behavior_latent"))),
]
BIT_IDS = ["smallest", "pulse_echo2", "throughout_from0", "last_step", "N17_J15", "N17_J16", "N17_J17", "N17_J33", "five_nets", "actor_only",
           "critic_only", "tanh", "no_beh", "two_overridden", "nothing_knocked", "strided_view", "expanded_over_jobs", "inplace_fc1",
           "no_base_override", "base_of_a_second_source"]
FP64_CASES = [BIT_CASES[i] for i in (1, 2, 6, 8, 9, 10, 11, 13)]
FP64_IDS = [BIT_IDS[i] for i in (1, 2, 6, 8, 9, 10, 11, 13)]
DIMS, WIN = KT.DIMS, KT.WIN


# ------------------------------------------------------------------------------------------------ the overrides and the copies
def make_override(case, J, win, keys=(AL,), base=None, view="contig", seed=5):
    """-> (override dict name -> [E, H, nA, J, N, w], override_base dict name -> [E, H, nA, N, w]) on the case's device, drawn on the
    latent's scale.  ``view``: "contig"; "strided" (job axis outermost in memory, three NaN floats behind every entity row, a NaN
    margin at both ends); "expand" (one vector for every job: stride 0 over the job axis)"""
    nA, E, S, N = case.dims[:4]
    start, D, H = win
    widths = dict(case.widths)
    gen = torch.Generator().manual_seed(seed + 7 * J + sum(win))
    over, over_base = {}, {}
    for k in keys:
        w = widths[k]
        if view == "strided":
            shape = (J, E, H, nA, N, w + 3)
            n = int(np.prod(shape))
            flat = torch.full((n + 8,), float("nan"))
            flat[4:4 + n].view(shape)[..., :w] = torch.randn(J, E, H, nA, N, w, generator=gen) * 2
            over[k] = flat.to(case.device)[4:4 + n].view(shape)[..., :w].permute(1, 2, 3, 0, 4, 5)
            assert not over[k].is_contiguous()
        elif view == "expand":
            over[k] = (torch.randn(E, H, nA, 1, N, w, generator=gen) * 2).to(case.device).expand(E, H, nA, J, N, w)
            assert over[k].stride(3) == 0
        else:
            over[k] = (torch.randn(E, H, nA, J, N, w, generator=gen) * 2).to(case.device)
    for k in (keys if base is None else base):
        over_base[k] = (torch.randn(E, H, nA, N, widths[k], generator=gen) * 2).to(case.device)
    return over, over_base


def base_fields(case, win, over_base, fields=None):
    """a copy of the episode fields with ``override_base`` written into the window"""
    start, D, H = win
    f = {k: v.clone() for k, v in (fields or case.f).items()}
    for k, v in over_base.items():
        f[k][:, start:start + H] = v.cpu()
    return f


def job_fields(case, j, q, win, over, over_base, knocked, baseline=None, fields=None):
    """a copy of the episode fields as job slot q (entity j) sees them: the overridden fields hold override[..., q, :, :] over the whole
    window; a job -1 reads the base override of a source it has no override of; the entity's columns of ``knocked`` are replaced in
    steps start .. start + D - 1"""
    start, D, H = win
    f = KT.window_fields(case, j, start, D, knocked, baseline, fields)
    for k, v in over_base.items():
        if j < 0 and k not in over:
            f[k][:, start:start + H] = v.cpu()
    for k, v in over.items():
        f[k][:, start:start + H] = v[:, :, :, q].cpu()
    return f


def _knocked(case, over, sources=None):
    return tuple(k for k in (case.names if sources is None else sources) if k not in over)


def run(case, win, over, over_base, **kw):
    return KT.run(case, win, override=over, override_base=over_base or None, **kw)


def op_overrides(case, over, over_base, win, extra_base_slot=False):
    """the method's dicts as the op's per-source lists [nA, E, H, J, N, w] / [nA, E, H, N, w]; ``extra_base_slot``: one more job slot
    whose vector is the base's (its override_base, or the batch's own window) -- a slot that repeats column 15"""
    start, D, H = win
    ovs, ovb = [], []
    for k in case.names:
        ov = over.get(k)
        if ov is not None and extra_base_slot:
            b = over_base[k] if k in over_base else case.f[k][:, start:start + H].to(case.device)
            ov = torch.cat([ov, b.unsqueeze(3)], 3)
        ovs.append(None if ov is None else ov.permute(2, 0, 1, 3, 4, 5))
        ovb.append(None if k not in over_base else over_base[k].permute(2, 0, 1, 3, 4))
    return ovs, ovb


# ------------------------------------------------------------------------------------------------ 1: the bits of a re-run
def check_same_bits(device, dims, J, win, opt, ch):
    """1: every job slot against the trace of its explicit copy, bit for bit, at every step; the base against the trace of the copy
    with override_base written in; kl, dlogp, dvalue and shift_sq against knockout_trace_checks._host_pairs' fp32 host loops"""
    case = _case(dims, opt, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    which = opt.get("which", "both")
    keys, sources = ch.get("keys", (AL,)), ch.get("sources")
    jobs = job_list(N, J)
    over, over_base = make_override(case, J, win, keys, ch.get("base"), ch.get("view", "contig"))
    knocked = _knocked(case, over, sources)
    keep = os.environ.get("IPLAN_NO_FC1_PACK")
    if ch.get("inplace"):
        os.environ["IPLAN_NO_FC1_PACK"] = "1"
    try:
        got = run(case, win, over, over_base, entities=jobs, which=which, want=ALL_WANT, sources=sources)
        w = {"actor": 0, "critic": 1, "both": 2}[which]
        ojobs = jobs + [-1]
        ovs, ovb = op_overrides(case, over, over_base, win, extra_base_slot=True)
        op = KT.op_call(case, ojobs, win, which=w, knock=tuple(k in knocked for k in case.names), override=ovs, override_base=ovb,
                        **(dict(packed=None) if ch.get("inplace") else {}))
    finally:
        if ch.get("inplace"):
            if keep is None:
                del os.environ["IPLAN_NO_FC1_PACK"]
            else:
                os.environ["IPLAN_NO_FC1_PACK"] = keep
    assert got["knocked"] == tuple(jobs) and got["sources"] == knocked and got["window"] == win and got["overridden"] == tuple(
        k for k in case.names if k in over)
    for k in PAIR_KEYS:
        on = which != ("actor" if k in ("dvalue", "values_ko", "state_shift_critic", "h_critic_ko") else "critic")
        assert (k in got) == on, (k, which)
        if on:
            assert got[k].shape[:4] == (E, H, nA, J), (k, got[k].shape)
    base = KT.window_trace(case, base_fields(case, win, over_base), start, H, which)
    for mine, theirs in KT.BASE_OF:
        if mine in got:
            assert torch.equal(_bits(got[mine]), _bits(base[theirs])), (dims, win, mine, "the base chain differs from the trace with override_base")
    moved = False
    for q, j in enumerate(jobs):
        if ch.get("view") == "expand" and j in jobs[:q]:
            continue                                                          # (the same entity and the same vector: the same copy)
        ref = KT.window_trace(case, job_fields(case, j, q, win, over, over_base, knocked), start, H, which)
        KT._assert_job_is_trace(got, q, ref, (dims, win, opt, ch, "slot", q, "job", j))
        moved = moved or any(not torch.equal(ref[t], base[t]) for _, t in KT.BASE_OF if t in ref)
    assert moved, "no job differs from the base: the case checks nothing"
    host = KT._host_pairs(case, op, ojobs, win, w)                           # (its base: the first -1 slot -- the extra one, if no job is -1)
    if -1 in jobs:                                                            # a job -1 has a vector of its own: the base is the LAST slot
        host = _host_pairs_last(case, op, ojobs, win, w)
    for k, ref in host.items():
        assert np.array_equal(op[k].cpu().numpy().view(np.int32), ref.view(np.int32)), (dims, win, opt, ch, k, "differs from the fp32 host loop")
        name = k.replace("shift_sq", "state_shift")
        mine = got[name].permute(2, 0, 1, 3)
        theirs = torch.from_numpy(ref[..., :J]).to(mine.device)
        assert torch.equal(_bits(mine), _bits(theirs.sqrt() if k.startswith("shift") else theirs)), (dims, win, opt, ch, name, "method != op")
    return {}


def _host_pairs_last(case, op, jobs, win, which):
    """knockout_trace_checks._host_pairs with the base taken from the last slot: the job list reversed, the outputs flipped along the
    job axis, so that its ``jobs.index(-1)`` finds that slot"""
    flip = {k: (v.flip(3) if torch.is_tensor(v) and v.dim() >= 4 and k != "probs" else v) for k, v in op.items()}
    host = KT._host_pairs(case, flip, jobs[::-1], win, which)
    return {k: np.ascontiguousarray(v[:, :, :, ::-1]) for k, v in host.items()}


# ------------------------------------------------------------------------------------------------ 2: reduction to what exists
def check_reduces_to_knockout_trace(device, dims=DIMS, win=WIN):
    """2: the batch's own attention_latent broadcast over the jobs as the override, no base override: knockout_trace's bits"""
    case = get_case(dims, device)
    nA, E, S, N = dims[:4]
    start, D, H = win
    jobs = job_list(N, N + 2)
    srcs = tuple(k for k in case.names if k != AL)
    own = case.f[AL][:, start:start + H].to(device).unsqueeze(3).expand(-1, -1, -1, len(jobs), -1, -1)
    got = run(case, win, {AL: own}, None, entities=jobs, sources=srcs, want=ALL_WANT + ("summary",))
    ref = KT.run(case, win, entities=jobs, sources=srcs, want=ALL_WANT + ("summary",))
    assert got["sources"] == ref["sources"] == srcs and got["overridden"] == (AL,) and "overridden" not in ref
    KT._same(got, ref, "the batch's own latent as the override", [k for k in ref if torch.is_tensor(ref[k])])
    assert bool((ref["kl"] != 0).any())
    return {}


def check_agrees_with_knockout(device, dims=DIMS, start=1):
    """2: H = 1 agrees with knockout(steps=start, override=...) from the same state within 1e-5 (check_agrees_with_knockout's bound)"""
    case = get_case(dims, device)
    N = dims[3]
    win = (start, 1, 1)
    jobs = job_list(N, N + 1)
    over, _ = make_override(case, len(jobs), win)
    got = run(case, win, over, None, entities=jobs)
    one = case.mac.knockout(case.batch, entities=jobs, steps=slice(start, start + 1), override=over)
    _sync(device)
    worst = {}
    for k in ("kl", "dlogp", "dvalue"):
        diff = (got[k] - one[k]).abs().max().item()
        print("knockout_trace(override) vs knockout(override) at H = 1:", k, diff)
        _worse(worst, k + "_vs_knockout", diff)
        assert diff <= TOL, (k, diff)
    assert bool((got["kl"] > 0).any())
    return worst


# ------------------------------------------------------------------------------------------------ 3: exact zeros
def check_exact_zeros(device, dims, win, opt):
    """3: a job whose override rows equal override_base and whose knocked values equal the originals (an entity whose columns are
    already zero in the knocked steps, and a job -1) has kl = dlogp = dvalue = state_shift = +0.0 at every step and the base's bits"""
    case = _case(dims, opt, device)
    N = dims[3]
    start, D, H = win
    key = AL if AL in case.names else "history"
    f = KT.window_fields(case, 1, start, D, tuple(k for k in case.names if k != key))
    jobs = [1, 0, -1, 1] + job_list(N, 13)                                    # 17 slots: the unchanged job in both tiles
    over, over_base = make_override(case, len(jobs), win, (key,))
    same = [q for q, j in enumerate(jobs) if j in (1, -1) and q not in (4, 5)]   # (some slots of those jobs keep a vector of their own)
    for q in same:
        over[key][:, :, :, q] = over_base[key]
    got = run(case, win, over, over_base, batch=case.to_batch(f), entities=jobs, want=ALL_WANT)
    for q in same:
        for k in ("kl", "dlogp", "dvalue", "state_shift_actor", "state_shift_critic"):
            v = got[k][:, :, :, q]
            assert v.shape[1] == H and bool((v == 0).all()) and not bool(torch.signbit(v).any()), (k, "is not exactly +0.0 on an unchanged job", q, jobs[q])
        for mine, theirs in (("probs_ko", "probs"), ("logp_ko", "logp"), ("values_ko", "values"), ("greedy", "greedy_base")):
            assert torch.equal(_bits(got[mine][:, :, :, q]), _bits(got[theirs])), (mine, "differs from the base", q, jobs[q])
        assert not bool(got["flip"][:, :, :, q].any())
    rest = [q for q in range(len(jobs)) if q not in same]
    for k in ("dvalue", "kl", "state_shift_actor", "state_shift_critic"):
        assert bool((got[k][:, :, :, rest] != 0).all(3).any()), (k, "the changed jobs moved nothing")
    assert bool((got["state_shift_critic"][:, :, :, rest] != 0).all()), "an override that differs at every step leaves a step unmoved"
    return {}


# ------------------------------------------------------------------------------------------------ 4: the social chain
def _social_setup(device, tmp_path, E=3, N=4, seed=4, plant=None, win=None):
    from iplan_amd import synth
    from tests.predict_checks import _e2e_args, _loaded_policy
    args = _e2e_args(device, max_vehicle_num=N, episode_limit=6)
    pol, _, _ = _loaded_policy(args, tmp_path, 23)
    mac = make_mac(args, 19)
    f = synth.make_episode_fields(args, E, seed=seed, terminated_p=0.1)
    f["avail_actions"].scatter_(-1, f["actions"], 1)
    if plant is not None:                                                     # an unseen vehicle: its rows already equal the zero baseline
        start, D, H = win
        f["history"][:, start:start + D, :, plant] = 0.0
        f["behavior_latent"][:, start - 1:start + D, :, plant] = 0.0
    T1 = f["history"].shape[1]
    return args, pol, mac, f, synth.DictBatch(f, E, T1).to(device), T1


def _by_hand(pol, mac, f, batch, win, device, entities=None, **kw):
    """the two public calls: attention_knockout_trace on the rollout's alignment, then knockout_trace with its latents"""
    start, D, H = win
    dv = lambda t: t.to(device)                                                    # noqa: E731
    g = pol.attention_knockout_trace(dv(f["history"][:, 1:]), dv(f["behavior_latent"][:, :-1]), hidden0=dv(f[AL][:, start - 1]), entities=entities,
                                     start=start - 1, duration=D, horizon=H, want=("latent_ko", "shift"))
    res = mac.knockout_trace(batch, entities=entities, start=start, duration=D, horizon=H, override={AL: g["latent_ko"]}, override_base={AL: g["latent"]}, **kw)
    _sync(device)
    return g, res


def check_social(device, tmp_path):
    """4: knockout_trace(social=) equals the two public calls made by hand, bit for bit; the same at a max_workspace_mb that forces
    two environment chunks and two job chunks or more (asserted); start = 1 is the smallest window, start = 0 is refused; a planted
    unseen vehicle gives exact zeros in both halves"""
    E, N = 3, 4
    win = (2, 1, 3)
    args, pol, mac, f, batch, T1 = _social_setup(device, tmp_path, E, N, plant=2, win=win)
    nA = args.n_agents
    want = ALL_WANT + ("summary", "latent_shift")
    for w_ in (win, (1, 2, 2)):
        start, D, H = w_
        g, ref = _by_hand(pol, mac, f, batch, w_, device, want=ALL_WANT + ("summary",))
        got = mac.knockout_trace(batch, start=start, duration=D, horizon=H, social=pol, want=want)
        _sync(device)
        assert got["overridden"] == (AL,) and AL not in got["sources"] and got["sources"] == ref["sources"]
        KT._same(got, ref, ("social", w_), [k for k in ref if torch.is_tensor(ref[k])])
        assert got["latent_shift"].shape == (E, H, nA, N, N) and torch.equal(_bits(got["latent_shift"]), _bits(g["latent_shift"]))
        assert bool((got["kl"] != 0).any()) and bool((got["latent_shift"] != 0).any())
        if w_ == win:                                                         # the planted vehicle: zeros in the GAT half and in the policy half
            assert bool((got["latent_shift"][..., 2] == 0).all()), "the unseen vehicle moved a latent"
            for k in ("kl", "dlogp", "dvalue", "state_shift_actor", "state_shift_critic"):
                v = got[k][:, :, :, 2]
                assert bool((v == 0).all()) and not bool(torch.signbit(v).any()), (k, "is not exactly +0.0 for the unseen vehicle")
                assert bool((got[k][:, :, :, [0, 1, 3]] != 0).any()), (k, "nothing else moved either")
    # chunks: the byte counts of one (environment, job) pair's two halves, as the method counts them
    start, D, H = win
    A, n_act = args.attention_dim, args.n_actions
    gat_env = 4 * nA * H * (2 * N * (N - 1) + N * A)
    gat_job = 4 * nA * H * (N * A + N)
    job = KT._pair_bytes(nA, H, n_act) + 2 * nA * H * 4 * L.AC_TRACE_GI * 16 // 15 + 1 + gat_job
    full = mac.knockout_trace(batch, start=start, duration=D, horizon=H, social=pol, want=want)
    calls = []
    real = ops.policy_knockout_trace

    def counted(actor_arena, critic_arena, which, spec, En, *a, **kw):
        calls.append((En, len(a[3])))
        return real(actor_arena, critic_arena, which, spec, En, *a, **kw)
    ops.policy_knockout_trace = counted
    try:
        for mb, chunks in (((gat_env + 2 * job) / 2 ** 20, (E, 2)), (1e-9, (E, N))):
            calls.clear()
            part = mac.knockout_trace(batch, start=start, duration=D, horizon=H, social=pol, want=want, max_workspace_mb=mb)
            _sync(device)
            assert len(calls) == chunks[0] * chunks[1] and chunks[0] >= 2 and chunks[1] >= 2, (mb, calls)
            assert all(En == 1 and Jn == N // chunks[1] for En, Jn in calls), calls
            KT._same(part, full, ("social, max_workspace_mb", mb), [k for k in full if torch.is_tensor(full[k])])
    finally:
        ops.policy_knockout_trace = real
    for bad in (dict(start=0), dict(start=1, override={AL: torch.zeros(E, H, nA, N, N, A)}), dict(start=1, social_kw=dict(want=("shift",))),
                dict(start=1, entities=[0, -1]), dict(start=1, override_base={AL: torch.zeros(E, H, nA, N, A)})):
        try:
            mac.knockout_trace(batch, **{**dict(duration=1, horizon=H, social=pol), **bad})
        except ValueError:
            continue
        raise AssertionError(f"knockout_trace(social=) accepted {sorted(bad)}")
    # social_kw reaches the GAT half: its sources, and its noise together with deterministic=False
    nz = torch.randn(nA, E, H, N, N - 1, 2, generator=torch.Generator().manual_seed(1)).to(device)
    kw = dict(sources=("history",), noise=nz, deterministic=False, tau=1.0)
    dv = lambda t: t.to(device)                                                    # noqa: E731
    g = pol.attention_knockout_trace(dv(f["history"][:, 1:]), dv(f["behavior_latent"][:, :-1]), hidden0=dv(f[AL][:, start - 1]), start=start - 1,
                                     duration=D, horizon=H, want=("latent_ko",), **kw)
    ref = mac.knockout_trace(batch, start=start, duration=D, horizon=H, override={AL: g["latent_ko"]}, override_base={AL: g["latent"]})
    got = mac.knockout_trace(batch, start=start, duration=D, horizon=H, social=pol, social_kw=kw)
    KT._same(got, ref, "social_kw", [k for k in ref if torch.is_tensor(ref[k])])
    assert not torch.equal(got["kl"], full["kl"])
    return {}


# ------------------------------------------------------------------------------------------------ 5: fp64
def _refs(case, jobs, win, over, over_base, knocked):
    """the fp64 and the fp32 oracle chains of the base and of every job slot -> {dtype: dict}, knockout_trace_checks.check_vs_fp64's"""
    start, D, H = win
    J = len(jobs)
    av = case.f["avail_actions"][:, start:start + H].permute(2, 0, 1, 3) != 0
    tgt = case.f["actions"][:, start:start + H, :, 0].permute(2, 0, 1).unsqueeze(-1)
    refs = {}
    for dt in (torch.float64, torch.float32):
        base = KT._oracle_chain(case, base_fields(case, win, over_base), start, H, dt)
        slots = [KT._oracle_chain(case, job_fields(case, j, q, win, over, over_base, knocked), start, H, dt) for q, j in enumerate(jobs)]
        st = lambda k: torch.stack([s[k] for s in slots], 3)                                    # noqa: E731  [nA, E, H, J, ..]
        tiny = 1e-300 if dt == torch.float64 else 1e-38
        lb, lk = base["probs"].clamp_min(tiny).log(), st("probs").clamp_min(tiny).log()
        r = dict(probs_ko=st("probs"), values_ko=st("values"), h_actor_ko=st("h_actor"), h_critic_ko=st("h_critic"))
        r["logp_full"] = lk.gather(-1, tgt.unsqueeze(3).expand(-1, -1, -1, J, -1))[..., 0]
        r["dlogp"] = r["logp_full"] - lb.gather(-1, tgt)[..., 0].unsqueeze(-1)
        r["kl"] = torch.where(av.unsqueeze(3), base["probs"].unsqueeze(3) * (lb.unsqueeze(3) - lk), torch.zeros_like(lk)).sum(-1)
        r["dvalue"] = r["values_ko"] - base["values"].unsqueeze(-1)
        r["state_shift_actor"] = (r["h_actor_ko"] - base["h_actor"].unsqueeze(3)).norm(dim=-1)
        r["state_shift_critic"] = (r["h_critic_ko"] - base["h_critic"].unsqueeze(3)).norm(dim=-1)
        r["base"] = base
        refs[dt] = r
    return refs, av


def check_vs_fp64(device, dims, J, win, opt, ch, kernel=True):
    """5: every float output against the fp64 oracle chain on the modified fields under the rule; greedy and flip away from fp64 ties.
    ``kernel=False``: the fp32 oracle alone in the library's place -- that the chosen seeds keep IT inside the caps"""
    case = _case(dims, opt, device if kernel else "cpu")
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    which = opt.get("which", "both")
    jobs = job_list(N, J)
    over, over_base = make_override(case, J, win, ch.get("keys", (AL,)), ch.get("base"))
    knocked = _knocked(case, over, ch.get("sources"))
    refs, av = _refs(case, jobs, win, over, over_base, knocked)
    r64, r32 = refs[torch.float64], refs[torch.float32]
    has = av.any(-1)
    if kernel:
        got = run(case, win, over, over_base, entities=jobs, which=which, want=ALL_WANT, sources=ch.get("sources"))
    else:
        got = {k: v.permute(1, 2, 0, *range(3, v.dim())) for k, v in r32.items() if k not in ("base", "logp_full")}
        got["logp_ko"] = r32["logp_full"].permute(1, 2, 0, 3)
        got["greedy"] = got["probs_ko"].argmax(-1)
        got["flip"] = got["greedy"] != r32["base"]["probs"].permute(1, 2, 0, 3).argmax(-1).unsqueeze(-1)
    worst = {}
    skipped = total = 0
    keys = [k for k in ("probs_ko", "logp_ko", "values_ko", "h_actor_ko", "h_critic_ko", "kl", "dlogp", "dvalue", "state_shift_actor", "state_shift_critic")
            if k in got]
    for i in range(nA):
        for key in keys:
            g = got[key][:, :, i].cpu()
            ref, ref32 = (r["logp_full" if key == "logp_ko" else key][i] for r in (r64, r32))
            if key in ("logp_ko", "dlogp"):
                g, ref, ref32 = g[has[i]], ref[has[i]], ref32[has[i]]
            err, e32 = _rel(g, ref), _rel(ref32, ref)
            bound = max(TOL, E32_FACTOR * e32)
            print((dims, win, opt, ch), "agent", i, key, "err", err, "e32", e32, "bound", bound)
            _worse(worst, key, err)
            _worse(worst, key + "_e32", e32)
            assert err <= bound, (dims, win, opt, ch, i, key, err, e32)
        if which != "critic":
            knocked_steps = torch.zeros(H, dtype=torch.bool)
            knocked_steps[:D] = True
            changed = (torch.tensor([j >= 0 for j in jobs])[None, None, :] & (av[i].sum(-1) >= 2)[:, :, None]) & knocked_steps[None, :, None]
            if n_act > 1 and bool(changed.any()):
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


# ------------------------------------------------------------------------------------------------ 6: independence, repeatability
def check_independence(device, reps=2, dims=(1, 2, 4, 7, 5, 5), win=(1, 2, 3)):
    """6: a slot's bits do not change under permuted, duplicated or subsetted jobs (each with its override rows), J or E split by a
    tiny max_workspace_mb, a shorter H (a prefix), packed or in-place fc1 operands, or the outputs asked for; each ``reps`` times"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    jobs = list(range(N))
    over, over_base = make_override(case, N, win)
    want = ALL_WANT + ("summary",)
    full = run(case, win, over, over_base, want=want)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(2)).tolist()
    pick = lambda idx: {k: v[:, :, :, idx] for k, v in over.items()}           # noqa: E731
    for _ in range(reps):
        KT._same(run(case, win, over, over_base, want=want), full, "repeat")
        for idx in (perm, [3, 3, 6, 3, 0] * 4, [4], jobs + jobs + jobs[:3]):   # 7, 20, 1 and 17 slots: another lane, another tile
            part = run(case, win, pick(idx), over_base, entities=idx, want=ALL_WANT)
            KT._same(KT._slots(part, list(range(len(idx)))), KT._slots(full, idx), ("jobs", idx))
            KT._same(part, full, ("base with jobs", idx), BASE_KEYS)
        job = KT._pair_bytes(nA, H, n_act) + 2 * nA * H * 4 * L.AC_TRACE_GI * 16 // 15 + 1
        for mb in (3 * E * job / 2 ** 20, N * job / 2 ** 20, 1e-9):            # J split; E split; one pair per launch
            KT._same(run(case, win, over, over_base, want=want, max_workspace_mb=mb), full, ("max_workspace_mb", mb))
        for h in range(D, H):
            short = run(case, (start, D, h), {k: v[:, :h] for k, v in over.items()}, {k: v[:, :h] for k, v in over_base.items()}, want=ALL_WANT)
            KT._same(short, {k: (v[:, :h] if torch.is_tensor(v) else v) for k, v in full.items()}, ("horizon", h), PAIR_KEYS + BASE_KEYS)
        keep = os.environ.get("IPLAN_NO_FC1_PACK")
        os.environ["IPLAN_NO_FC1_PACK"] = "1"
        try:
            assert case.mac.fc1_pack.get(None) is None
            inplace = run(case, win, over, over_base, want=want)
        finally:
            if keep is None:
                del os.environ["IPLAN_NO_FC1_PACK"]
            else:
                os.environ["IPLAN_NO_FC1_PACK"] = keep
        KT._same(inplace, full, "packed != in place")
        for w in ((), ("probs_ko",), ("values_ko", "summary"), ("h_critic_ko",)):
            KT._same(run(case, win, over, over_base, want=w), full, ("want", w))
        for which in ("actor", "critic"):
            KT._same(run(case, win, over, over_base, which=which, want=ALL_WANT), full, ("which", which))
    ovs, ovb = op_overrides(case, over, over_base, win)
    op_full = KT.op_call(case, jobs, win, override=ovs, override_base=ovb)
    for w in (("kl",), ("dvalue",), ("base",), ("shift_sq",), ("greedy_ko", "probs_ko"), ("logp_ko", "values_ko", "dlogp", "h_ko")):
        KT._same(KT.op_call(case, jobs, win, want=w, override=ovs, override_base=ovb), op_full, ("op want", w))
    return {}


# ------------------------------------------------------------------------------------------------ 7: ownership (the op)
def check_ownership(device, dims, J, win):
    """7: outputs carved out of sentinel-filled, NaN-edged buffers keep their surroundings, every owned element is written, outputs not
    asked for stay untouched; the H-deep gi_ko of the call, pre-filled with NaN, is written in the slots of real columns only"""
    case = get_case(dims, device)
    nA, E, S, N = dims[:4]
    start, D, H = win
    jobs = job_list(N, J)
    over, over_base = make_override(case, J, win)
    kw = dict(zip(("override", "override_base"), op_overrides(case, over, over_base, win)))
    shapes = KT._op_shapes(case, J, win)
    ref = KT.op_call(case, jobs, win, **kw)
    assert set(ref) == set(shapes)
    for which, want in ((2, OP_WANT), (2, ("kl",)), (0, ("base", "probs_ko", "h_ko")), (1, ("dvalue", "values_ko", "shift_sq"))):
        bufs = KT._sentinels(shapes, device)
        got = KT.op_call(case, jobs, win, which=which, want=want, out={k: v[2] for k, v in bufs.items()}, **kw)
        owned = {k for w in want for k in KT.OWNED.get(w, (w,)) if (k in KT.ACTOR_KEYS and which != 1) or (k not in KT.ACTOR_KEYS and which != 0)}
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
    b2 = KT._sentinels(shapes, device, 0.25)
    JT = (J + 14) // 15
    assert ops.policy_knockout_trace_gi_floats(2, nA, E, H, D, J, override=True) == 2 * nA * E * H * JT * 16 * L.AC_TRACE_GI
    gi = torch.full((2, nA, E, H, JT, 16, L.AC_TRACE_GI), float("nan"), device=device)
    out = {k: v[2] for k, v in b2.items()}
    out["gi_ko"] = gi
    res = KT.op_call(case, jobs, win, want=OP_WANT + ("gi_ko",), out=out, **kw)
    assert res["gi_ko"].shape == (2, nA, E, H, JT, 16, L.AC_TRACE_GI)
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
def check_touches_nothing(device):
    """8: parameters, gradient entries, the optimisers' state, hidden_states, the batch, the override tensors and the generator states
    are bit-identical before and after knockout_trace(override=); a train() after it gives the bits of one without it"""
    results = []
    for with_call in (False, True):
        args, mac, learner, batch = SC._learner(device)
        torch.manual_seed(83)
        for arena in (mac.actor_arena, mac.critic_arena):
            arena.grad.zero_()
        if with_call:
            for arena in (mac.actor_arena, mac.critic_arena):
                arena.grad.fill_(0.7071)
            watched = [t for t in SC._state_tensors(learner) if t.device.type == torch.device(device).type]
            assert len(watched) > 8, len(watched)
            before = [t.clone() for t in watched]
            fields = {k: v.clone() for k, v in batch.data.items()}
            E, T1, nA, N = batch.data["history"].shape[:4]
            H, A = 3, args.attention_dim
            gen = torch.Generator().manual_seed(9)
            ov = torch.randn(E, H, nA, N, N, A, generator=gen).to(device)
            ovb = torch.randn(E, H, nA, N, A, generator=gen).to(device)
            ov0, ovb0 = ov.clone(), ovb.clone()
            states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, np.random.get_state()[1].copy())
            mac.hidden_states = "untouched"
            res = mac.knockout_trace(batch, start=1, duration=1, horizon=H, want=ALL_WANT + ("summary",), override={AL: ov}, override_base={AL: ovb})
            _sync(device)
            assert torch.isfinite(res["kl"]).all() and torch.isfinite(res["dvalue"]).all() and res["dvalue"].abs().sum() > 0
            assert torch.equal(torch.get_rng_state(), states[0]) and np.array_equal(np.random.get_state()[1], states[2])
            if states[1] is not None:
                assert torch.equal(torch.cuda.get_rng_state(), states[1])
            assert mac.hidden_states == "untouched"
            mac.hidden_states = None
            assert torch.equal(_bits(ov), _bits(ov0)) and torch.equal(_bits(ovb), _bits(ovb0)), "an override tensor was written"
            for t, b in zip(watched, before):
                assert torch.equal(_bits(t), _bits(b)), ("a tensor of the learner changed", tuple(t.shape))
            for arena in (mac.actor_arena, mac.critic_arena):
                assert torch.equal(arena.grad, torch.full_like(arena.grad, 0.7071)), "a gradient entry was written"
                arena.grad.zero_()
            for k, v in fields.items():
                assert torch.equal(batch.data[k], v), (k, "the batch was written")
        learner.train(0)
        _sync(device)
        results.append((mac.actor_arena.data.clone(), mac.critic_arena.data.clone()))
    (a0, c0), (a1, c1) = results
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    return {}


# ------------------------------------------------------------------------------------------------ 9: the method, the entry point
def check_methods(device, tmp_path):
    """9: on a loaded checkpoint; numpy-backed and device-backed batches and overrides agree"""
    dims, win = (2, 3, 4, 3, 5, 5), (1, 2, 3)
    src = get_case(dims, device)
    case = copy.copy(src)
    case.mac = make_mac(src.args, 77)
    src.mac.save_models(str(tmp_path))
    assert not torch.equal(case.mac.actor_arena.data, src.mac.actor_arena.data)
    case.mac.load_models([str(tmp_path)])
    nA, E, S, N = dims[:4]
    jobs = [2, -1, 0, 1, 2]
    from iplan_amd import synth
    over, over_base = make_override(case, len(jobs), win, (AL, "behavior_latent"))
    want = ALL_WANT + ("summary",)
    r_dev = run(case, win, over, over_base, entities=jobs, want=want)
    KT._same(r_dev, run(src, win, over, over_base, entities=jobs, want=want), "the loaded checkpoint differs from its source")
    np_batch = synth.DictBatch({k: v.numpy() for k, v in case.f.items()}, E, case.T1)
    r_np = KT.run(case, win, batch=np_batch, entities=jobs, want=want, override={k: v.cpu().numpy() for k, v in over.items()},
                  override_base={k: v.cpu().numpy() for k, v in over_base.items()})
    meta = ("knocked", "sources", "window", "overridden")
    assert r_dev["overridden"] == (AL, "behavior_latent") and r_dev["sources"] == ("history",)
    for k, v in r_dev.items():
        if k in meta:
            assert r_np[k] == v
            continue
        assert isinstance(r_np[k], np.ndarray) and torch.is_tensor(v) and v.device.type == torch.device(device).type, k
        assert np.array_equal(r_np[k], v.cpu().numpy()), (k, "numpy-backed and device-backed calls differ")
    ref = KT.window_trace(case, job_fields(case, 2, 0, win, over, over_base, ("history",)), win[0], win[2])
    KT._assert_job_is_trace(r_dev, 0, ref, "the loaded checkpoint")
    return {}


def check_method_refusals(device, dims=DIMS):
    """9: ValueError before anything is launched"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    mac = case.mac
    H = 2
    A = dict(case.widths)[AL]
    ok = torch.zeros(E, H, nA, N, N, A)
    okb = torch.zeros(E, H, nA, N, A)

    def refuses(m=mac, batch=case.batch, **kw):
        try:
            m.knockout_trace(batch, **{**dict(start=1, horizon=H), **kw})
        except ValueError:
            return
        raise AssertionError(f"knockout_trace accepted {sorted(kw)}")
    refuses(override={AL: ok[:, :1]})
    refuses(override={AL: ok[..., :A - 1]})
    refuses(override={AL: ok}, entities=[0, 1])
    refuses(override={AL: okb})
    refuses(override={AL: ok}, override_base={AL: ok})
    refuses(override={AL: ok}, override_base={AL: okb[:, :1]})
    refuses(override={"intent": ok})
    refuses(override={AL: ok}, override_base={"intent": okb})
    refuses(override=ok)
    refuses(override_base={AL: okb})
    refuses(override={"history": torch.zeros(E, H, nA, N, N, d)}, override_base={AL: okb}, horizon=H + 1)
    refuses(social_kw=dict(tau=1.0))
    refuses(want=("latent_shift",))
    refuses(override={AL: ok}, want=("latent_shift",))
    no_gat = get_case((1, 2, 4, 3, 5, 5), device, (("gat", False),))
    refuses(no_gat.mac, no_gat.batch, override={AL: torch.zeros(2, H, 1, 3, 3, A)})                 # an absent source
    refuses(no_gat.mac, no_gat.batch, override={"history": torch.zeros(2, H, 1, 3, 3, d)}, override_base={AL: torch.zeros(2, H, 1, 3, A)})
    refuses(no_gat.mac, no_gat.batch, social=object())                                              # social needs GAT_enable
    refuses(social=object(), start=0)
    refuses(social=object(), override={AL: ok})
    refuses(social=object(), social_kw=dict(want=("shift",)))
    refuses(social=object(), social_kw=("tau",))
    got = mac.knockout_trace(case.batch, start=1, horizon=H, override={AL: ok.to(device)}, sources=(AL,))
    assert got["sources"] == () and got["overridden"] == (AL,) and got["kl"].shape == (E, H, nA, N)
    return {}


def check_bad_arguments(device, dims=DIMS, win=WIN):
    """9 (the entry point): each invalid descriptor is refused by the host-side check with IPLAN_EINVAL / IPLAN_EALIGN and a message
    that names the entry; nothing is launched, so the sentinel-filled outputs stay as they were"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    start, D, H = win
    mac = case.mac
    jobs = [0, 2, -1]
    over, over_base = make_override(case, len(jobs), win)
    ovs, ovb = op_overrides(case, over, over_base, win)
    good = KT.op_call(case, jobs, win, override=ovs, override_base=ovb)
    bufs = KT._sentinels(KT._op_shapes(case, len(jobs), win), device)
    r = mac._rows(case.batch, start, H)
    ha, hc = r.field("rnn_states_actors", torch.float32)[:, start], r.field("rnn_states_critics", torch.float32)[:, start]
    lib = ops._lib(None)
    EINVAL, EALIGN = _codes(), KT._code("IPLAN_EALIGN")
    fn = lib.c.iplan_ac_knockout_chain
    c = L.AcKnockoutChainArgs()
    a = c.kt
    ops._ac_rows(a.base, mac.actor_arena, mac.critic_arena, 2, r.spec, E, H, nA)
    ops._fill_acnet(a.base.actor, mac.actor_arena, L.ACTOR_PARAM_ORDER, n_act)
    ops._fill_acnet(a.base.critic, mac.critic_arena, L.CRITIC_PARAM_ORDER, 1)
    a.base.hidden0_actor, a.base.hidden0_critic = ha.data_ptr(), hc.data_ptr()
    a.base.h0_s_net, a.base.h0_s_chain = ha.stride(1), ha.stride(0)
    gi_ko = torch.zeros(2 * nA * E * H * 16 * L.AC_TRACE_GI + 4, device=device)
    a.gi_ko = gi_ko.data_ptr()
    a.D, a.J = D, len(jobs)
    j_host = (L.C.c_int32 * 3)(*jobs)
    j_dev = torch.tensor(jobs, dtype=torch.int32, device=device)
    a.jobs, a.jobs_host = j_dev.data_ptr(), L.C.cast(j_host, L.C.c_void_p)
    for k in range(3):
        a.knock[k] = 1
    a.kl, a.dvalue = bufs["kl"][2].data_ptr(), bufs["dvalue"][2].data_ptr()
    a.h_ko_actor = bufs["h_ko_actor"][2].data_ptr()
    ops._chain_overrides(c, r.spec, nA, E, H, len(jobs), ovs[1].device, ovs, ovb)
    assert c.override_src[1] and c.override_base[1] and not c.override_src[0]

    def refused(args_ref, code=EINVAL, **fields):
        keep_f = {}
        for k, v in fields.items():
            obj, name = c, k
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
        assert rc == code and rc < 0 and "iplan_ac_knockout_chain" in msg, (fields, rc, msg)
        return msg

    refused(None)
    ref = L.C.byref(c)
    # everything iplan_ac_knockout_trace refuses
    refused(ref, **{"kt.base.which": 3})
    refused(ref, **{"kt.base.n_agents": 0})
    refused(ref, **{"kt.base.E": 0})
    refused(ref, **{"kt.base.S": 0})
    assert "D=" in refused(ref, **{"kt.D": 0})
    assert "D=" in refused(ref, **{"kt.D": H + 1})
    assert "phases" in refused(ref, **{"kt.base.phases": 3})
    refused(ref, **{"kt.base.feat.N": 65})
    refused(ref, **{"kt.base.feat.T": H + 1})
    refused(ref, **{"kt.base.feat.T_phys": H - 1})
    refused(ref, **{"kt.base.feat.n_id": -1})
    assert "source 0" in refused(ref, **{"kt.base.feat.src[0]": None})
    refused(ref, **{"kt.J": 0})
    refused(ref, **{"kt.jobs": None})
    refused(ref, **{"kt.jobs_host": None})
    bad = (L.C.c_int32 * 3)(0, N, -1)
    assert "job 1" in refused(ref, **{"kt.jobs_host": L.C.cast(bad, L.C.c_void_p)})
    bad2 = (L.C.c_int32 * 3)(0, 1, -2)
    assert "job 2" in refused(ref, **{"kt.jobs_host": L.C.cast(bad2, L.C.c_void_p)})
    assert "too many" in refused(ref, **{"kt.base.E": 2 ** 27})
    assert "absent" in refused(ref, **{"kt.base.feat.w[2]": 0})
    assert "absent" in refused(ref, **{"kt.base.feat.w[2]": 0, "kt.knock[2]": 0, "kt.baseline[2]": 64})
    assert "base's outputs" in refused(ref, **{"kt.base.entropy": 64})
    assert "base's outputs" in refused(ref, **{"kt.base.h_last_actor": 64})
    assert "base's outputs" in refused(ref, **{"kt.base.h_all_critic": 64})
    refused(ref, **{"kt.base.actor.n_out": 17})
    refused(ref, **{"kt.base.actor.params": None})
    refused(ref, **{"kt.base.critic.n_out": 2})
    refused(ref, **{"kt.base.critic.params": None})
    assert "no output" in refused(ref, **{"kt.kl": None, "kt.dvalue": None, "kt.h_ko_actor": None})
    assert "no output" in refused(ref, **{"kt.kl": None, "kt.h_ko_actor": None, "kt.base.which": 0})
    # the chain's own
    assert "gi_ko" in refused(ref, **{"kt.gi_ko": None})
    assert "base.gi" in refused(ref, **{"kt.base.gi": gi_ko.data_ptr()})
    assert "absent source 2" in refused(ref, **{"kt.base.feat.w[2]": 0, "kt.knock[2]": 0, "override_src[2]": c.override_src[1]})
    assert "absent source 2" in refused(ref, **{"kt.base.feat.w[2]": 0, "kt.knock[2]": 0, "override_base[2]": c.override_base[1]})
    for name in ("ov_s_job", "ov_s_net", "ov_s_chain", "ov_s_step", "ov_s_ent"):
        assert "negative override stride" in refused(ref, **{name + "[1]": -1}), name
    for name in ("ovb_s_net", "ovb_s_chain", "ovb_s_step", "ovb_s_ent"):
        assert "negative base override stride" in refused(ref, **{name + "[1]": -1}), name
    assert "iplan_ac_knockout_trace is the entry" in refused(ref, **{"override_src[1]": None})
    assert "iplan_ac_knockout_trace is the entry" in refused(ref, **{"override_src[1]": None, "override_base[1]": None})
    for field, v in (("kt.gi_ko", gi_ko.data_ptr() + 4), ("kt.h_ko_actor", a.h_ko_actor + 4), ("kt.h_ko_critic", 68), ("kt.base.packed_actor", 68),
                     ("kt.base.packed_critic", 72)):
        assert "aligned" in refused(ref, code=EALIGN, **{field: v}), field
    assert "aligned" in refused(ref, code=EALIGN, **{"kt.base.packed_s_net": 2})

    def raises(**kw):
        args = dict(override=ovs, override_base=ovb)
        args.update(kw)
        try:
            KT.op_call(case, jobs, win, out={k: v[2] for k, v in bufs.items()}, **args)
        except AssertionError:
            return
        raise AssertionError(f"ops.policy_knockout_trace accepted {sorted(kw)}")
    raises(override=[None, None, None])                                       # a base override alone
    raises(override=[None, ovs[1][:, :, :1], None])
    raises(override=[None, ovs[1].double(), None])
    raises(override=[None, ovs[1][:, :, :, :2], None])
    raises(override=[None, torch.zeros(*ovs[1].shape[:5], 2 * ovs[1].shape[5], device=device)[..., ::2], None])    # a strided innermost axis
    raises(override_base=[None, ovb[1][:, :1], None])
    raises(override=[None, None, None, ovs[1]])
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(_bits(buf.cpu()), _bits(sent)), (k, "a refused call wrote an output")
    KT._same(KT.op_call(case, jobs, win, override=ovs, override_base=ovb), good, "after the refusals")
    return {}


def check_abi():
    """9: the size registry of the active library knows the new struct, the ctypes mirror has its size, the entry is exported"""
    lib = ops._lib(None)
    assert "IplanAcKnockoutChainArgs" in L.STRUCT_MIRRORS and "iplan_ac_knockout_chain" in L.ENTRY_POINTS
    n = lib.c.iplan_sizeof(b"IplanAcKnockoutChainArgs")
    assert n > 0 and n == L.C.sizeof(L.STRUCT_MIRRORS["IplanAcKnockoutChainArgs"]), (n, L.C.sizeof(L.STRUCT_MIRRORS["IplanAcKnockoutChainArgs"]))
    assert hasattr(lib.c, "iplan_ac_knockout_chain")
    return {}
