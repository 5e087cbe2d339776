"""TEST INFRASTRUCTURE: policy knock-out attribution (csrc/policy_knockout.hip, ops.policy_knockout, DcntrlMAC.knockout) on whatever
library is active -- the host emulator in tests/test_emu_policy_knockout.py, the gfx950 build in tests/test_gpu_policy_knockout.py.

Ground truth 1 (bits): job j on the original batch against the BASE result of the same method on an explicit copy of the batch with
entity j's selected columns replaced, and (1e-5) against a one-step ``_trace`` on that copy.
Ground truth 2 (fp64): oracle.actor_logits / oracle.critic_value on the modified input rows (saliency_checks.build_rows), the recorded
state held.  Rule: error = max|got - ref64| / max(1, max|ref64|) over the pairs of one agent, bound = max(1e-5,
E32_FACTOR x the same oracle run in fp32 against fp64); the same rule for kl, dlogp and dvalue against the fp64 quantities.
Two places where fp32 and fp64 part by construction are left out of the fp64 comparison and nowhere else: logp of a row with NO
available action (every logit is the constant -1e10, and -1e10 + log n rounds to -1e10 in fp32: the trace's convention gives 0, fp64
-log n), and the KL floor of 1e-6, which is asked of pairs whose row has at least two available actions (with one, every
distribution is the same point mass).
The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors."""
import copy
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from iplan_amd.controllers.dcntrl_controller import _esn
from oracle import iplan_oracle as O
from tests import saliency_checks as SC
from tests.oracle_checks import E32_FACTOR, _rel
from tests.policy_trace_checks import _args, _bits, _codes, _e2e_args, _params, _sync, _worse, assert_out_refused, make_mac

TOL = 1e-5
M = 64
GAP = 1e-5                # fp64 top-two gap below which a row's greedy action is not compared
SKIP_CAP = 0.05           # ... and the largest share of such rows
KL_FLOOR = 1e-6
PAIR_KEYS = ("kl", "dlogp", "dvalue", "greedy", "flip", "probs_ko", "logp_ko", "values_ko")
ALL_WANT = ("kl", "probs_ko", "logp_ko", "values_ko")
OP_WANT = ("base", "kl", "dlogp", "dvalue", "greedy_ko", "probs_ko", "logp_ko", "values_ko")

# (nA, E, S, N, d, n_actions), J, options.  A tile holds 15 jobs and the base: J = 1, 15, 16, 17, 33 are one tile with one job, a full
# tile, two tiles with one job in the second, ..., three tiles.  d = 5: an entity's history columns straddle lanes and k-tiles; the
# latents are 32 and 8 wide.  E x S = 1, and 5 / 6 rows: with one tile per row a ragged last workgroup of four tiles.
KERNEL_CASES = [
    ((1, 1, 1, 2, 5, 5), 1, {}),
    ((1, 5, 1, 3, 5, 5), 15, {}),
    ((2, 3, 2, 3, 5, 5), 16, {}),
    ((1, 3, 1, 17, 5, 5), 17, {}),
    ((1, 1, 2, 17, 5, 5), 33, {}),
    ((5, 2, 1, 3, 5, 5), 4, {}),
    ((1, 3, 1, 3, 5, 5), 5, dict(gat=False)),
    ((1, 3, 1, 3, 5, 5), 5, dict(beh=False)),
    ((1, 2, 2, 17, 5, 5), 3, dict(gat=False, beh=False)),
    ((2, 3, 1, 3, 5, 1), 4, {}),
    ((2, 3, 1, 3, 5, 5), 4, dict(tanh=True)),
    ((1, 2, 2, 2, 5, 5), 3, dict(tanh=True, gat=False)),
    ((2, 3, 2, 3, 5, 5), 4, dict(which="actor")),
    ((2, 3, 2, 3, 5, 5), 4, dict(which="critic")),
]
CASE_IDS = ["one_row_J1", "rows5_J15", "two_agents_J16", "N17_J17", "N17_J33", "five_agents", "no_gat", "no_beh", "history_only", "one_action",
            "tanh", "tanh_no_gat_N2", "actor_only", "critic_only"]
FP64_CASES = [KERNEL_CASES[i] for i in (2, 3, 5, 6, 8, 9, 10, 12, 13)]
FP64_IDS = [CASE_IDS[i] for i in (2, 3, 5, 6, 8, 9, 10, 12, 13)]
_NAMES = ("history", "attention_latent", "behavior_latent")
SOURCE_CASES = [(tuple(k for b, k in enumerate(_NAMES) if m >> b & 1), base) for m in range(1, 8) for base in (False, True)]     # each flag set


def job_list(N, J):
    """J jobs in [-1, N): the entities from the last (whose history columns end in the ragged last k-tile) down to 0, then -1, then
    the same again -- every entity and -1 as far as J reaches, duplicates beyond"""
    cycle = list(range(N - 1, -1, -1)) + [-1]
    return [cycle[i % (N + 1)] for i in range(J)]


class Case:
    """a DcntrlMAC with spread-out parameters and an episode batch [E, S + 1, nA, ...] (T_phys > T): dense random features, avail with
    random zeros and the recorded action always available -- except row (0, 0), where ONLY the recorded action is available, and the
    last row (E - 1, S - 1) of a batch with three rows or more, where NONE is"""

    def __init__(self, dims, device, seed=0, **opt):
        from iplan_amd import synth
        nA, E, S, N, d, n_act = dims
        self.dims, self.device = dims, device
        self.args = _args(device, nA, N, d, n_act, S, **opt)
        a = self.args
        self.mac = make_mac(a, 41 + seed)
        f = synth.make_episode_fields(a, E, seed=11 + seed + sum(dims), terminated_p=0.2)
        gen = torch.Generator().manual_seed(300 + seed + sum(dims))
        f["history"] = torch.rand(f["history"].shape, generator=gen) * 8 - 4
        f["history"][..., 0] = (torch.rand(f["history"].shape[:-1], generator=gen) < 0.8).float()       # the presence column
        f["attention_latent"] = torch.randn(f["attention_latent"].shape, generator=gen) * 2
        av = (torch.rand(f["avail_actions"].shape, generator=gen) < 0.6).int()
        av.scatter_(-1, f["actions"], 1)
        av[0, 0] = 0
        av[0, 0].scatter_(-1, f["actions"][0, 0], 1)
        if E * S >= 3:
            av[E - 1, S - 1] = 0
        f["avail_actions"] = av
        self.f = f
        self.T1 = S + 1
        self.widths = self.mac._widths()
        self.names = tuple(k for k, _ in self.widths)
        self.batch = self.to_batch(f)

    def to_batch(self, f):
        from iplan_amd import synth
        return synth.DictBatch(f, self.dims[1], self.T1).to(self.device)

    def run(self, batch=None, steps=None, **kw):
        S = self.dims[2]
        res = self.mac.knockout(self.batch if batch is None else batch, steps=slice(0, S) if steps is None else steps, **kw)
        _sync(self.device)
        return res

    def knocked_fields(self, j, sources=None, baseline=None, fields=None):
        """a copy of the episode fields with entity j's columns of ``sources`` replaced at every step (j = -1: a plain copy)"""
        f = {k: v.clone() for k, v in self.f.items()}
        if fields:
            f.update(fields)
        if j >= 0:
            for k in (self.names if sources is None else sources):
                f[k][:, :, :, j] = 0.0 if baseline is None or baseline.get(k) is None else baseline[k].to(f[k].dtype)
        return f


@functools.lru_cache(maxsize=None)
def get_case(dims, device, opt=(), seed=0):
    return Case(dims, device, seed=seed, **dict(opt))


def _case(dims, opt, device):
    return get_case(dims, device, tuple(sorted((k, v) for k, v in opt.items() if k != "which")))


def _baseline(case, gen_seed=3):
    gen = torch.Generator().manual_seed(gen_seed)
    return {k: torch.randn(w, generator=gen) for k, w in case.widths}


def _copy_base(case, f, which, S, steps=None):
    """the base result of the method on an explicit copy of the batch"""
    return case.run(batch=case.to_batch(f), entities=[-1], which=which, steps=steps)


def _assert_job_is_copy(got, q, ref, which, what):
    """slot q of ``got`` carries the bits of ``ref``'s base result"""
    pairs = []
    if which != "critic":
        pairs += [("probs_ko", "probs"), ("logp_ko", "logp"), ("greedy", "greedy_base")]
    if which != "actor":
        pairs += [("values_ko", "values")]
    for mine, theirs in pairs:
        g = got[mine][:, :, :, q]
        assert torch.equal(_bits(g), _bits(ref[theirs])), (what, mine, "differs from the base result of the modified copy")


def _assert_near_trace(case, f, got, q, which, worst, what):
    """the same slot within 1e-5 of one-step traces from the recorded states on the modified copy"""
    S = case.dims[2]
    batch = case.to_batch(f)
    for s in range(S):
        res, _, _ = case.mac._trace(batch, s, 1, None, which, ("probs", "greedy", "logp", "values"), False)
        _sync(case.device)
        for mine, theirs in (("probs_ko", "probs"), ("logp_ko", "logp"), ("values_ko", "values")):
            if theirs not in res:
                continue
            t = res[theirs][:, :, 0]
            t = t.permute(1, 0, 2) if t.dim() == 3 else t.t()
            diff = (got[mine][:, s, :, q] - t).abs().max().item()
            _worse(worst, mine + "_vs_trace", diff)
            assert diff <= TOL, (what, mine, s, diff)
        if "greedy" in res:
            p = res["probs"][:, :, 0].permute(1, 0, 2)
            top = p.topk(min(2, p.shape[-1]), -1).values
            clear = (top[..., 0] - top[..., -1] >= 2 * GAP) | (p.shape[-1] == 1)
            same = got["greedy"][:, s, :, q] == res["greedy"][:, :, 0].t()
            assert bool((same | ~clear).all()), (what, "greedy differs from the trace's on a row without a tie", s)


# ------------------------------------------------------------------------------------------------ 1: the bits of a rerun
def check_same_bits(device, dims, J, opt):
    """1: every job against the base result of an explicit copy, bit for bit, and against one-step traces at 1e-5; shapes and dtypes"""
    case = _case(dims, opt, device)
    nA, E, S, N, d, n_act = dims
    which = opt.get("which", "both")
    jobs = job_list(N, J)
    got = case.run(entities=jobs, which=which, want=ALL_WANT)
    assert got["knocked"] == tuple(jobs) and got["sources"] == case.names
    for k in PAIR_KEYS:
        on = which != ("actor" if k in ("dvalue", "values_ko") else "critic")
        assert (k in got) == on, (k, which)
        if on:
            assert got[k].shape[:4] == (E, S, nA, J), (k, got[k].shape)
    if which != "critic":
        assert got["greedy"].dtype == torch.int64 and got["flip"].dtype == torch.bool and got["probs_ko"].shape == (E, S, nA, J, n_act)
        assert torch.equal(got["target_action"].cpu(), case.f["actions"][:, :S, :, 0])
        av = case.f["avail_actions"][:, :S]
        some = (av.sum(-1, keepdim=True) > 0).unsqueeze(3)
        assert bool((got["probs_ko"].cpu()[((av == 0).unsqueeze(3) & some).expand(-1, -1, -1, J, -1)] == 0).all()), "an unavailable action has probability"
    worst = {}
    done = set()
    for q, j in enumerate(jobs):
        if j in done:
            continue
        done.add(j)
        f = case.knocked_fields(j)
        ref = _copy_base(case, f, which, S)
        _assert_job_is_copy(got, q, ref, which, (dims, opt, "job", j))
        if len(done) <= 3:
            _assert_near_trace(case, f, got, q, which, worst, (dims, opt, "job", j))
    for q, j in enumerate(jobs):                                             # duplicates of a job carry the same bits
        p = jobs.index(j)
        for k in PAIR_KEYS:
            if k in got and p != q:
                assert torch.equal(_bits(got[k][:, :, :, q]), _bits(got[k][:, :, :, p])), (k, "two slots of the same job differ", p, q)
    return worst


def check_sources_and_baseline(device, sources, with_baseline, dims=(2, 3, 2, 3, 5, 5)):
    """1: each knock flag combination, with zeros and with a non-zero baseline"""
    case = get_case(dims, device)
    S, N = dims[2], dims[3]
    base = _baseline(case) if with_baseline else None
    got = case.run(sources=sources, baseline=base, want=ALL_WANT)
    assert got["sources"] == tuple(sources)
    full = case.run(want=ALL_WANT)
    if len(sources) < 3 or with_baseline:
        assert not torch.equal(got["values_ko"], full["values_ko"]), "the selection changed nothing"
    for j in range(N):
        ref = _copy_base(case, case.knocked_fields(j, sources, base), "both", S)
        _assert_job_is_copy(got, j, ref, "both", (sources, with_baseline, j))
    return {}


def check_no_flag(device, dims=(2, 3, 2, 3, 5, 5)):
    """1: the op with every knock flag off (the method has no such call): every job is the base, with and without a baseline"""
    case = get_case(dims, device)
    N = dims[3]
    jobs = list(range(N)) + [-1]
    base = [b.to(device) for b in _baseline(case).values()]
    for bl in (None, base):
        got = op_call(case, jobs, knock=[False, False, False], baseline=bl)
        for k in ("kl", "dlogp", "dvalue"):
            assert bool((got[k] == 0).all()), (k, "is not exactly 0 with no source knocked")
        for mine, theirs in (("probs_ko", "probs"), ("logp_ko", "logp"), ("values_ko", "values"), ("greedy_ko", "greedy")):
            assert torch.equal(_bits(got[mine]), _bits(got[theirs].unsqueeze(3).expand_as(got[mine]))), (mine, "differs from the base")
    _same(op_call(case, jobs[:1], knock=[False, False, False], want=("base",)), op_call(case, jobs[:1], want=("base",)), "the base depends on the flags")
    return {}


def _override(case, J, key="attention_latent", seed=5):
    """a per-job source [E, S, nA, J, N, w] as a strided view inside a NaN-filled buffer: three NaN floats behind every entity row, a NaN
    margin at both ends of the storage, the job axis outermost in memory"""
    nA, E, S, N = case.dims[:4]
    w = dict(case.widths)[key]
    gen = torch.Generator().manual_seed(seed)
    shape = (J, E, S, nA, N, w + 3)
    n = int(np.prod(shape))
    flat = torch.full((n + 8,), float("nan"))
    mem = flat[4:4 + n].view(shape)
    mem[..., :w] = torch.randn(J, E, S, nA, N, w, generator=gen)
    return flat.to(case.device)[4:4 + n].view(shape)[..., :w].permute(1, 2, 3, 0, 4, 5)


def _op_override(case, J, key="attention_latent"):
    """the same for the op: [nA, E, S, J, N, w]"""
    return _override(case, J, key).permute(2, 0, 1, 3, 4, 5)


def check_override(device, dims=(2, 3, 2, 3, 5, 5)):
    """1: a per-job override against copies whose field IS the override slice, the other sources knocked as usual; an overridden
    source is not knocked as well"""
    case = get_case(dims, device)
    nA, E, S, N = dims[:4]
    jobs = [1, -1, 0, 2, 1]
    for key in ("attention_latent", "history"):
        ov = _override(case, len(jobs), key)
        assert not ov.is_contiguous()
        got = case.run(entities=jobs, override={key: ov}, want=ALL_WANT)
        for q, j in enumerate(jobs):
            field = case.f[key].clone()
            field[:, :S] = ov[:, :, :, q].cpu()
            others = tuple(k for k in case.names if k != key)
            ref = _copy_base(case, case.knocked_fields(j, others, fields={key: field}), "both", S)
            _assert_job_is_copy(got, q, ref, "both", ("override", key, q, j))
    return {}


# ------------------------------------------------------------------------------------------------ 2: fp64
def _oracle(case, f, i, dtype, sl):
    """agent i on the rows of steps ``sl`` of fields ``f`` -> (log-probabilities [R, n_act], V [R])"""
    a = case.args
    ap, cp = _params(case.mac, dtype)
    x = SC.build_rows(SimpleNamespace(args=a, f=f), i, dtype, sl).flatten(0, 1)
    R = x.shape[0]
    ha = f["rnn_states_actors"][:, sl, i].reshape(R, M).to(dtype)
    hc = f["rnn_states_critics"][:, sl, i].reshape(R, M).to(dtype)
    av = f["avail_actions"][:, sl, i].reshape(R, -1)
    logits, _ = O.actor_logits(ap[i], x, ha, av, use_relu=a.use_ReLU)
    v, _ = O.critic_value(cp[i], x, hc, use_relu=a.use_ReLU)
    return torch.log_softmax(logits, -1), v[:, 0]


def _oracle_pairs(case, jobs, i, dtype, sl):
    """-> dict of [R, J, ..]: probs_ko, logp_all, values_ko, kl, dvalue and the base's [R, ..]"""
    lb, vb = _oracle(case, case.f, i, dtype, sl)
    av = case.f["avail_actions"][:, sl, i].flatten(0, 1) != 0
    out = dict(lp=[], v=[], kl=[])
    cache = {}
    for j in jobs:
        if j not in cache:
            lk, vk = _oracle(case, case.knocked_fields(j), i, dtype, sl) if j >= 0 else (lb, vb)
            kl = torch.where(av, lb.exp() * (lb - lk), torch.zeros_like(lb)).sum(-1)
            cache[j] = (lk, vk, kl)
        for k, t in zip(("lp", "v", "kl"), cache[j]):
            out[k].append(t)
    res = {k: torch.stack(v, 1) for k, v in out.items()}
    res.update(lb=lb, vb=vb, av=av)
    return res


def check_vs_fp64(device, dims, J, opt):
    """2: probs_ko, logp_ko, values_ko, kl, dlogp and dvalue under the rule; greedy_ko = the oracle's argmax away from ties; the
    comparison is not vacuous (fp64 KL > 1e-6 on every pair with a changed row that has a choice)"""
    case = _case(dims, opt, device)
    nA, E, S, N, d, n_act = dims
    which = opt.get("which", "both")
    jobs = job_list(N, J)
    got = case.run(entities=jobs, which=which, want=ALL_WANT)
    sl = slice(0, S)
    worst = {}
    skipped = total = 0
    for i in range(nA):
        r64, r32 = (_oracle_pairs(case, jobs, i, dt, sl) for dt in (torch.float64, torch.float32))
        R = E * S
        tgt = case.f["actions"][:, sl, i, 0].reshape(R, 1, 1).expand(-1, J, -1)
        has = r64["av"].any(-1)                                               # rows with an available action
        refs = {}
        if which != "critic":
            refs["probs_ko"] = tuple(r["lp"].exp() for r in (r64, r32))
            refs["logp_ko"] = tuple(r["lp"].gather(-1, tgt)[..., 0][has] for r in (r64, r32))
            refs["dlogp"] = tuple((r["lp"].gather(-1, tgt)[..., 0] - r["lb"].gather(-1, tgt[:, 0])) for r in (r64, r32))
            refs["kl"] = (r64["kl"], r32["kl"])
        if which != "actor":
            refs["values_ko"] = (r64["v"], r32["v"])
            refs["dvalue"] = tuple(r["v"] - r["vb"][:, None] for r in (r64, r32))
        for key, (ref, ref32) in refs.items():
            g = got[key][:, :, i].cpu().flatten(0, 1)
            if key == "logp_ko":
                g = g[has]
            err, e32 = _rel(g, ref), _rel(ref32, ref)
            bound = max(TOL, E32_FACTOR * e32)
            print((dims, opt), "agent", i, key, "err", err, "e32", e32, "bound", bound)
            _worse(worst, key, err)
            _worse(worst, key + "_e32", e32)
            assert err <= bound, (dims, opt, i, key, err, e32)
        if which != "critic":
            changed = torch.tensor([j >= 0 for j in jobs])[None, :] & (r64["av"].sum(-1) >= 2)[:, None]
            if n_act > 1:
                assert bool(changed.any()) and bool((r64["kl"][changed] > KL_FLOOR).all()), (dims, opt, i, "a changed pair has fp64 KL <= 1e-6", r64["kl"][changed].min().item())
            p64 = r64["lp"].exp()
            top = p64.topk(min(2, n_act), -1).values
            clear = (top[..., 0] - top[..., -1] >= GAP) if n_act > 1 else torch.ones(R, J, dtype=torch.bool)
            same = got["greedy"][:, :, i].cpu().flatten(0, 1) == p64.argmax(-1)
            assert bool((same | ~clear).all()), (dims, opt, i, "greedy_ko differs from the fp64 argmax away from a tie")
            skipped += int((~clear & has[:, None]).sum())
            total += int(has.sum()) * J
    if which != "critic":
        worst["greedy_skipped_share"] = skipped / max(total, 1)
        assert skipped <= SKIP_CAP * total, (dims, opt, "too many rows at an fp64 tie", skipped, total)
    return worst


# ------------------------------------------------------------------------------------------------ 3: exact zeros
def check_exact_zeros(device, dims, opt, mode):
    """3: a job that replaces values by the same values has kl = dlogp = dvalue = 0.0 exactly and the base's bits; the -1 slots are
    the base.  mode "zeros": entity 1's columns are zero in the batch; "baseline": they hold the baseline rows"""
    case = _case(dims, opt, device)
    nA, E, S, N = dims[:4]
    base = _baseline(case, 9) if mode == "baseline" else None
    f = case.knocked_fields(1, None, base)
    jobs = [1, 0, -1, 1] + job_list(N, 13)                                    # 17 slots: the unchanged job in both tiles
    got = case.run(batch=case.to_batch(f), entities=jobs, baseline=base, want=ALL_WANT)
    for q, j in enumerate(jobs):
        if j not in (1, -1):
            continue
        for k in ("kl", "dlogp", "dvalue"):
            assert bool((got[k][:, :, :, q] == 0).all()), (mode, k, "is not exactly 0 on an unchanged row", q, j)
        for mine, theirs in (("probs_ko", "probs"), ("logp_ko", "logp"), ("values_ko", "values"), ("greedy", "greedy_base")):
            assert torch.equal(_bits(got[mine][:, :, :, q]), _bits(got[theirs])), (mode, mine, "differs from the base", q, j)
        assert not bool(got["flip"][:, :, :, q].any())
    assert bool((got["dvalue"][:, :, :, 1] != 0).any()) and bool((got["kl"][:, :, :, 1] != 0).any()), "the changed job moved nothing"
    return {}


# ------------------------------------------------------------------------------------------------ 4: independence, repeatability
def _same(a, b, what, keys=None):
    for k in (keys or sorted(set(a) & set(b))):
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def _slots(res, idx):
    return {k: v[:, :, :, idx] for k, v in res.items() if k in PAIR_KEYS}


def check_independence(device, dims=(1, 2, 2, 7, 5, 5)):
    """4: a slot's bits do not change under permuted, duplicated or subsetted jobs, another J, the chunk size, steps=, packed or
    in-place fc1 operands, or which outputs were asked for"""
    case = get_case(dims, device)
    nA, E, S, N = dims[:4]
    full = case.run(want=ALL_WANT + ("summary",))
    base_keys = ("logp", "values", "probs", "target_action", "greedy_base")
    gen = torch.Generator().manual_seed(2)
    perm = torch.randperm(N, generator=gen).tolist()
    for jobs in (perm, perm[:5], [4], [3, 3, 6, 3, -1, 0] * 6, [j % N for j in range(16)]):
        part = case.run(entities=jobs, want=ALL_WANT)
        idx = [j for j in jobs if j >= 0]
        pos = [q for q, j in enumerate(jobs) if j >= 0]
        _same(_slots(part, pos), _slots(full, idx), ("jobs", jobs))
        _same(part, full, ("base with jobs", jobs), base_keys)
    # chunk sizes: one environment and four jobs per launch, one job per launch
    pair = nA * S * (4 * 3 + 8 + 4 * (2 + 5))
    for mb in (4 * pair / 2 ** 20, 1e-9):
        _same(case.run(want=ALL_WANT + ("summary",), max_workspace_mb=mb), full, ("max_workspace_mb", mb))
    for s0, s1 in ((0, 1), (1, 2)):
        part = case.run(steps=slice(s0, s1), want=ALL_WANT)
        _same(part, {k: (v[:, s0:s1] if torch.is_tensor(v) and v.dtype != torch.float64 else v) for k, v in full.items()}, ("steps", s0, s1),
              PAIR_KEYS + base_keys)
    one = case.run(steps=1, want=ALL_WANT)
    _same(one, {k: (v[:, 1] if torch.is_tensor(v) and v.dtype != torch.float64 else v) for k, v in full.items()}, "steps=int", PAIR_KEYS + base_keys)
    keep = os.environ.get("IPLAN_NO_FC1_PACK")
    os.environ["IPLAN_NO_FC1_PACK"] = "1"                                    # Fc1Pack.get returns None: the arena is read in place
    try:
        assert case.mac.fc1_pack.get(None) is None
        inplace = case.run(want=ALL_WANT)
    finally:
        if keep is None:
            del os.environ["IPLAN_NO_FC1_PACK"]
        else:
            os.environ["IPLAN_NO_FC1_PACK"] = keep
    _same(inplace, full, "packed != in place")
    for want in ((), ("probs_ko",), ("values_ko", "summary")):
        _same(case.run(want=want), full, ("want", want))
    for which in ("actor", "critic"):
        _same(case.run(which=which, want=ALL_WANT), full, ("which", which))
    op_full = op_call(case, list(range(N)), want=OP_WANT)
    for want in (("kl",), ("dvalue",), ("base",), ("greedy_ko", "probs_ko"), ("logp_ko", "values_ko", "dlogp")):
        _same(op_call(case, list(range(N)), want=want), op_full, ("op want", want))
    return {}


def check_repeatable(device, reps, dims=(1, 2, 2, 17, 5, 5)):
    """4: ``reps`` calls give the same bits"""
    case = get_case(dims, device)
    first = case.run(want=ALL_WANT + ("summary",))
    for _ in range(reps):
        _same(case.run(want=ALL_WANT + ("summary",)), first, "repeat")
    return {}


# ------------------------------------------------------------------------------------------------ 5: ownership (the op)
def _poisoned(t, pad=5, lead=4):
    """``t`` copied into the middle of a NaN-filled buffer: the same values, the last axis padded, the storage with a NaN margin"""
    shape = tuple(t.shape[:-1]) + (t.shape[-1] + pad,)
    n = int(np.prod(shape))
    mem = torch.full((n + 2 * lead,), float("nan"), dtype=t.dtype, device=t.device)
    view = mem[lead:lead + n].view(shape)[..., :t.shape[-1]]
    view.copy_(t)
    return view


def op_call(case, jobs, which=2, want=OP_WANT, knock=None, baseline=None, override=None, out=None, poison=False, args_only=False, **over):
    """ops.policy_knockout on the case's rows with the recorded states and actions; ``poison``: every float input inside NaN"""
    mac, S = case.mac, case.dims[2]
    nA = case.dims[0]
    r = mac._rows(case.batch, 0, S)
    ha, hc = r.field("rnn_states_actors", torch.float32)[:, r.sl], r.field("rnn_states_critics", torch.float32)[:, r.sl]
    spec = r.spec
    if poison:
        srcs = []
        for t, w, _, _ in spec.sources:                                      # [E, S, nA, N, w] -> rows of N * w floats inside NaN
            v = _poisoned(t.reshape(*t.shape[:3], -1))
            srcs.append((v, w, v.stride(2), v.stride(1)))
        spec = ops.AcFeatureSpec(spec.N, srcs, n_actions=spec.n_actions, last_action=None if spec.last_action is None else spec.last_action.contiguous(),
                                 la_strides=(0, 0) if spec.last_action is None else (1, nA), n_id=spec.n_id, T=S, T_phys=S)
        ha, hc = _poisoned(ha, 16), _poisoned(hc, 16)
        baseline = None if baseline is None else [None if b is None else _poisoned(b[None], 3)[0] for b in baseline]
    kw = dict(h_actor=ha, h_critic=hc, h_strides=_esn(ha), avail=r.avail, avail_strides=_esn(r.avail), target=r.acts, target_strides=_esn(r.acts),
              n_actions=mac.args.n_actions, knock=knock, baseline=baseline, override=override, want=want, packed=r.packed, out=out)
    kw.update(over)
    fn = ops.policy_knockout_args if args_only else ops.policy_knockout
    res = fn(mac.actor_arena, mac.critic_arena, which, spec, r.E, S, nA, jobs, **kw)
    _sync(case.device)
    return res


def _op_shapes(case, J):
    nA, E, S, N, d, n_act = case.dims
    pair = (nA, E, S, J)
    return dict(logp=(nA, E, S), values=(nA, E, S), target_action=(nA, E, S), greedy=(nA, E, S), probs=(nA, E, S, n_act), kl=pair, dlogp=pair, dvalue=pair,
                greedy_ko=pair, probs_ko=pair + (n_act,), logp_ko=pair, values_ko=pair)


def _sentinels(shapes, device, shift=0.0):
    bufs = {}
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        if k in ("target_action", "greedy", "greedy_ko"):
            sent = torch.arange(n + 64, dtype=torch.int64) * 7 + 1000
        else:
            sent = 0.5 + shift + (torch.arange(n + 64, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        bufs[k] = (sent, buf, buf[32:32 + n].view(shape))
    return bufs


OWNED = dict(base=("logp", "values", "target_action", "greedy", "probs"))
ACTOR_KEYS = ("logp", "target_action", "greedy", "probs", "kl", "dlogp", "greedy_ko", "probs_ko", "logp_ko")


def check_ownership(device, dims, J):
    """5: outputs carved out of sentinel-filled buffers, every float input surrounded by NaN: nothing outside the owned regions is
    written, every owned element is, outputs that were not asked for stay untouched, and no NaN is read"""
    case = get_case(dims, device)
    N = dims[3]
    jobs = job_list(N, J)
    base = [b.to(device) for b in _baseline(case).values()]
    ov = [None, _op_override(case, J), None]
    shapes = _op_shapes(case, J)
    ref = op_call(case, jobs, baseline=base, override=ov)
    assert set(ref) == set(shapes)
    for which, want in ((2, OP_WANT), (2, ("kl",)), (0, ("base", "probs_ko")), (1, ("dvalue", "values_ko")), (2, ("greedy_ko", "dlogp", "logp_ko"))):
        bufs = _sentinels(shapes, device)
        got = op_call(case, jobs, which=which, want=want, baseline=base, override=ov, out={k: v[2] for k, v in bufs.items()}, poison=True)
        owned = {k for w in want for k in OWNED.get(w, (w,)) if (k in ACTOR_KEYS and which != 1) or (k not in ACTOR_KEYS and which != 0)}
        assert set(got) == owned, (which, want, sorted(got), sorted(owned))
        for k, (sent, buf, view) in bufs.items():
            host = buf.cpu()
            if k not in owned:
                assert torch.equal(host, sent), (dims, which, want, k, "was not asked for and was written")
                continue
            assert torch.equal(_bits(view), _bits(ref[k])), (dims, k, "differs inside a padded buffer / beside NaN")
            n = view.numel()
            assert torch.equal(host[:32], sent[:32]) and torch.equal(host[32 + n:], sent[32 + n:]), (dims, k, "an element outside the owned region was written")
    b2 = _sentinels(shapes, device, 0.25)                                     # every owned element is written
    op_call(case, jobs, baseline=base, override=ov, out={k: v[2] for k, v in b2.items()})
    for k in shapes:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (dims, k, "an owned element was left unwritten")
    return {}


# ------------------------------------------------------------------------------------------------ 6: the method
def _host_summary(case, res, jobs, filled, S, presence_col=0):
    """the float64 host loop: means over the rows with weight filled, where the knocked entity is present"""
    nA = case.dims[0]
    hist = case.f["history"][:, :S].double()
    out = {k: np.zeros((nA, len(jobs))) for k in ("entity_kl", "entity_abs_dvalue", "flip_rate")}
    for i in range(nA):
        for q, j in enumerate(jobs):
            num, den = np.zeros(3), 0.0
            for e in range(hist.shape[0]):
                for s in range(S):
                    if j >= 0 and presence_col >= 0 and hist[e, s, i, j, presence_col] == 0:
                        continue
                    wt = float(filled[e, s])
                    den += wt
                    num += wt * np.array([float(res["kl"][e, s, i, q]), abs(float(res["dvalue"][e, s, i, q])), float(res["flip"][e, s, i, q])])
            for k, v in zip(out, num):
                out[k][i, q] = v / den if den > 0 else 0.0
    return out


def check_methods(device, tmp_path, steps):
    """6: on a loaded checkpoint, numpy and device inputs agree; one-step and sliced ``steps``; the summary against a float64 host loop"""
    dims = (2, 3, 3, 3, 5, 5)
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
    r_dev = case.run(steps=steps, entities=jobs, want=want)
    r_np = case.run(batch=np_batch, steps=steps, entities=jobs, want=want)
    _same(r_dev, src.run(steps=steps, entities=jobs, want=want), "the loaded checkpoint differs from its source")
    for k, v in r_dev.items():
        if k in ("knocked", "sources"):
            assert r_np[k] == v
            continue
        assert isinstance(r_np[k], np.ndarray) and torch.is_tensor(v) and v.device.type == torch.device(device).type, k
        assert np.array_equal(r_np[k], v.cpu().numpy()), (k, "numpy-backed and device-backed batches differ")
    one = isinstance(steps, int)
    sl = slice(steps, steps + 1) if one else steps
    Sn = sl.stop - sl.start
    assert r_dev["kl"].shape == ((E, nA, len(jobs)) if one else (E, Sn, nA, len(jobs)))
    whole = src.run(entities=jobs, want=want)
    _same(r_dev, {k: ((v[:, steps] if one else v[:, sl]) if torch.is_tensor(v) and v.dtype != torch.float64 else v) for k, v in whole.items()},
          "steps", PAIR_KEYS + ("logp", "values", "probs"))
    # the summary
    filled = case.f["filled"].reshape(E, -1)[:, sl].double()
    pairs = {k: (r_dev[k].unsqueeze(1) if one else r_dev[k]).cpu() for k in ("kl", "dvalue", "flip")}
    shifted = copy.copy(case)
    shifted.f = {k: (v[:, sl.start:] if k == "history" else v) for k, v in case.f.items()}
    host = _host_summary(shifted, pairs, jobs, filled, Sn)
    worst = {}
    for k, ref in host.items():
        assert r_dev[k].dtype == torch.float64 and r_dev[k].shape == (nA, len(jobs))
        err = np.abs(r_dev[k].cpu().numpy() - ref).max()
        _worse(worst, k, err)
        assert err <= 1e-12 * max(1.0, np.abs(ref).max()), (k, err)
    assert (host["entity_kl"] > 0).any()
    # presence_col < 0: every row counts (attention_knockout's rule)
    every = case.run(steps=steps, entities=jobs, want=("summary",), presence_col=-1)
    host_all = _host_summary(shifted, pairs, jobs, filled, Sn, presence_col=-1)
    for k, ref in host_all.items():
        err = np.abs(every[k].cpu().numpy() - ref).max()
        _worse(worst, k + "_every_row", err)
        assert err <= 1e-12 * max(1.0, np.abs(ref).max()), (k, "presence_col=-1", err)
    assert not np.array_equal(host_all["entity_abs_dvalue"], host["entity_abs_dvalue"]), "no entity is ever absent: the two summaries check the same"
    return worst


def check_chain(device, tmp_path, E=2):
    """6: attention_knockout's latent_ko of step t fed as the override of attention_latent at step t + 1 (the rollout's alignment:
    attention_latent[:, t + 1] = GAT(history[:, t + 1], attention_latent[:, t], behavior_latent[:, t])) equals the method on explicitly
    rebuilt batches, bit for bit"""
    from iplan_amd import synth
    from tests.predict_checks import _loaded_policy
    N = 3
    args = _e2e_args(device, max_vehicle_num=N)
    pol, _, _ = _loaded_policy(args, tmp_path, 23)
    mac = make_mac(args, 19)
    f = synth.make_episode_fields(args, E, seed=4, terminated_p=0.1)
    f["avail_actions"].scatter_(-1, f["actions"], 1)
    T1 = f["history"].shape[1]
    dv = lambda t: t.to(device)                                                    # noqa: E731
    batch = synth.DictBatch(f, E, T1).to(device)
    t0, t1 = 0, 2
    hist, beh, hid = dv(f["history"][:, t0 + 1:t1 + 1]), dv(f["behavior_latent"][:, t0:t1]), dv(f["attention_latent"][:, t0:t1])
    k = pol.attention_knockout(hist, beh, hid, want=("latent_ko",))
    lat_ko = k["latent_ko"]                                                        # [E, S, nA, J = N, N, A]
    got = mac.knockout(batch, steps=slice(t0 + 1, t1 + 1), override={"attention_latent": lat_ko}, want=ALL_WANT)
    _sync(device)
    moved = False
    for j in range(N):
        h2, b2 = hist.clone(), beh.clone()
        h2[:, :, :, j] = 0.0
        b2[:, :, :, j] = 0.0
        lat = pol.attention_knockout(h2, b2, hid, entities=[0])["latent"]          # the GAT on the explicit copy, nothing more knocked
        f2 = {kk: v.clone() for kk, v in f.items()}
        f2["history"][:, t0 + 1:t1 + 1, :, j] = 0.0
        f2["behavior_latent"][:, t0 + 1:t1 + 1, :, j] = 0.0
        f2["attention_latent"][:, t0 + 1:t1 + 1] = lat.cpu()
        ref = mac.knockout(synth.DictBatch(f2, E, T1).to(device), entities=[-1], steps=slice(t0 + 1, t1 + 1))
        _sync(device)
        _assert_job_is_copy(got, j, ref, "both", ("chain", j))
        moved = moved or not torch.equal(lat, k["latent"])
    assert moved, "no knocked latent differs from the base: the chain checks nothing"
    return {}


def check_touches_nothing(device, reps=1):
    """6: parameters, both arenas' gradient entries (pre-filled with a sentinel), the optimisers' state, hidden_states, the batch and
    the generator states are bit-identical before and after knockout(); a train() after knockout() gives the bits of one without it"""
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
                res = mac.knockout(batch, want=ALL_WANT + ("summary",), baseline={"history": torch.ones(args.obs_shape_single)})
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


# ------------------------------------------------------------------------------------------------ 7: refusals
def check_bad_arguments(device, dims=(2, 3, 2, 3, 5, 5)):
    """7 (the op): each invalid descriptor is refused by the host-side check with IPLAN_EINVAL and a message; ops.policy_knockout
    raises AssertionError for a wrong dtype or device, a job outside [-1, N), J = 0, an override or baseline on an absent source, a
    baseline of the wrong width, an override of the wrong shape, and a bad ``out=`` destination; nothing is launched, so the
    sentinel-filled outputs stay as they were"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    jobs = [0, 2, -1]
    good = op_call(case, jobs)
    bufs = _sentinels(_op_shapes(case, len(jobs)), device)
    a, res, keep = op_call(case, jobs, out={k: v[2] for k, v in bufs.items()}, args_only=True)
    lib = ops._lib(None)
    EINVAL = _codes()
    fn = lib.c.iplan_ac_knockout

    def refused(args_ref, **fields):
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
        assert rc == EINVAL and rc < 0 and "iplan_ac_" in msg, (fields, rc, msg)
        return msg

    assert "iplan_ac_knockout" in refused(None)
    ref = L.C.byref(a)
    assert "iplan_ac_knockout" in refused(ref, J=0)
    assert "iplan_ac_knockout" in refused(ref, J=-2)
    assert "iplan_ac_knockout" in refused(ref, jobs=None)
    assert "iplan_ac_knockout" in refused(ref, jobs_host=None)
    bad = (L.C.c_int32 * 3)(0, N, -1)
    assert "job 1" in refused(ref, jobs_host=L.C.cast(bad, L.C.c_void_p))
    bad2 = (L.C.c_int32 * 3)(0, 1, -2)
    assert "job 2" in refused(ref, jobs_host=L.C.cast(bad2, L.C.c_void_p))
    refused(ref, **{"base.feat.N": 65})                                      # the row description: iplan_ac_saliency's checks
    refused(ref, **{"base.E": 0})
    refused(ref, **{"base.S": 0})
    refused(ref, **{"base.which": 3})
    refused(ref, **{"base.h_actor": None})
    refused(ref, **{"base.h_critic": None})
    refused(ref, **{"base.target": None, "base.target_all": n_act})
    assert "base's outputs" in refused(ref, **{"base.entity_actor": 8})
    assert "base's outputs" in refused(ref, **{"base.act1_critic": 16})
    assert "absent" in refused(ref, **{"base.feat.w[2]": 0})                 # source 2 is knocked, and gone
    assert "absent" in refused(ref, **{"base.feat.w[2]": 0, "knock[2]": 0, "baseline[2]": 64})
    assert "absent" in refused(ref, **{"base.feat.w[2]": 0, "knock[2]": 0, "override_src[2]": 64})
    assert "stride" in refused(ref, **{"override_src[1]": 64, "ov_s_job[1]": -1})
    none = {k: None for k in ("probs_base", "greedy_base", "probs_ko", "logp_ko", "values_ko", "greedy_ko", "kl", "dlogp", "dvalue", "base.logp", "base.values",
                              "base.target_out")}
    assert "no output" in refused(ref, **none)
    assert "no output" in refused(ref, **{k: v for k, v in none.items() if k not in ("values_ko", "dvalue", "base.values")}, **{"base.which": 0})

    def raises(**kw):
        try:
            op_call(case, kw.pop("jobs", jobs), out={k: v[2] for k, v in bufs.items()}, **kw)
        except AssertionError:
            return
        raise AssertionError(f"ops.policy_knockout accepted {sorted(kw)}")
    raises(jobs=[])
    raises(jobs=[N])
    raises(jobs=[-2])
    dv = lambda t: t.to(device)                                                    # noqa: E731
    raises(baseline=[dv(torch.zeros(d + 1)), None, None])                          # the wrong width
    raises(baseline=[dv(torch.zeros(d, dtype=torch.float64)), None, None])         # the wrong dtype
    raises(baseline=[None, None, None, dv(torch.zeros(4))])                        # a source the rows do not have
    raises(knock=[True, True, True, True])
    raises(override=[None, None, None, _op_override(case, 3)])
    raises(override=[None, _op_override(case, 4), None])                              # J = 4 jobs' worth for 3 jobs
    raises(override=[None, _op_override(case, 3).double(), None])
    raises(override=[None, dv(torch.zeros(nA, E, S, 3, N, 64))[..., ::2], None])   # a strided innermost axis
    raises(want=("kl", "entity"))
    raises(want=())
    raises(which=1, want=("kl",))                                                  # nothing the critics provide
    raises(h_actor=None)
    raises(target=case.f["actions"][:, :S, :, 0].to(device).int())                 # the wrong dtype
    if torch.device(device).type == "cuda":
        raises(baseline=[torch.zeros(d), None, None])                              # the wrong device
    assert_out_refused(lambda out: op_call(case, jobs, out=out), bufs, ("kl", "greedy_ko", "probs", "logp"))
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(buf.cpu(), sent), (k, "a refused call wrote an output")
    _same(op_call(case, jobs), good, "after the refusals")
    del keep, res
    return {}


def check_method_refusals(device, dims=(2, 3, 2, 3, 5, 5)):
    """7 (the method): ValueError before anything is launched; layer_N / recurrent_N other than 1 raise NotImplementedError"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    mac = case.mac

    def refuses(exc=ValueError, **kw):
        try:
            mac.knockout(case.batch, **kw)
        except exc:
            return
        raise AssertionError(f"knockout accepted {kw}")
    refuses(entities=[])
    refuses(entities=[N])
    refuses(entities=[-2])
    refuses(sources=())
    refuses(sources=("history", "intent"))
    refuses(baseline={"intent": torch.zeros(3)})
    refuses(baseline=torch.zeros(d))
    refuses(baseline={"history": torch.zeros(d + 1)})
    refuses(baseline={"attention_latent": torch.zeros(8)})
    refuses(override={"intent": torch.zeros(3)})
    refuses(override={"attention_latent": torch.zeros(E, S + 1, nA, N - 1, N, 32)})
    refuses(override={"attention_latent": torch.zeros(E, S + 1, nA, N, N, 8)})
    refuses(want=("kl", "entity"))
    refuses(which="all")
    refuses(steps=slice(0, S, 2))
    refuses(steps=slice(1, 1))
    refuses(presence_col=d)
    refuses(presence_col=0.5)
    refuses(max_workspace_mb=0)
    no_gat = get_case((1, 3, 1, 3, 5, 5), device, (("gat", False),))
    for kw in (dict(sources=("attention_latent",)), dict(baseline={"attention_latent": torch.zeros(32)}),
               dict(override={"attention_latent": torch.zeros(3, 2, 1, 3, 3, 32)})):
        try:
            no_gat.mac.knockout(no_gat.batch, **kw)                           # an absent source
        except ValueError:
            continue
        raise AssertionError(f"knockout accepted {sorted(kw)} without a GAT")
    ok = mac.knockout(case.batch, entities=[1])
    assert ok["kl"].shape == (E, S + 1, nA, 1)
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


# ------------------------------------------------------------------------------------------------ 8: structure
def check_abi():
    """8: the size registry of the active library knows the new struct, and the ctypes mirror has its size"""
    lib = ops._lib(None)
    assert "IplanAcKnockoutArgs" in L.STRUCT_MIRRORS and "iplan_ac_knockout" in L.ENTRY_POINTS
    n = lib.c.iplan_sizeof(b"IplanAcKnockoutArgs")
    assert n > 0 and n == L.C.sizeof(L.STRUCT_MIRRORS["IplanAcKnockoutArgs"]), (n, L.C.sizeof(L.STRUCT_MIRRORS["IplanAcKnockoutArgs"]))
    return {}
