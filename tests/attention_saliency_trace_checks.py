"""TEST INFRASTRUCTURE: attention saliency through time (csrc/gat_saliency_trace.hip, ops.gat_saliency_trace,
Prediction_policy.attention_saliency_trace) on whatever library is active -- the host emulator in
tests/test_emu_attention_saliency_trace.py, the gfx950 build in tests/test_gpu_attention_saliency_trace.py.

Three judges:
  * the existing one-step kernel: every (target, lag) slot equals an ``ops.gat_saliency`` launch on the same record rows with the
    previous lag's ``hidden_grad`` as cotangent, bit for bit -- and on the public route ``attention_trace`` followed by lags + 1
    ``attention_saliency`` calls on shifted slices with the carries as tensor targets;
  * fp64 torch.autograd through lags + 1 chained oracle.gat_forward calls, one ego at a time (the scene replicated N times, as
    attention_saliency_checks.reference_scene does it), both ReLUs of every step on the kernel's own branches, the gate detached for
    ``gate="held"``.  Each lag slice is compared on its own, relative to its own size (``_grad_err``), so a wrong late lag cannot
    hide under lag 0's size.  Bound: max(1e-5, E32_FACTOR x e32), e32 = the fp32 oracle's own error against fp64 on the same slice,
    after asserting e32 <= 1e-4;
  * plain host restatements (the fp32 loop of carry_sq, the float64 numpy sums of lag_l1).
The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors it saw."""
import re
from unittest import mock

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import attention_saliency_checks as SC
from tests.attention_saliency_checks import A, E32_CAP, TOL, _bits, _gumbel, _sync, _worse
from tests.kernel_checks import _sentinel
from tests.oracle_checks import E32_FACTOR, _grad_err

TOUTS = ("grad", "pair_gl1", "pair_gxi", "input_grad", "carry", "carry_sq")
ONE_STEP = {"grad": "grad", "pair_gl1": "pair_gl1", "pair_gxi": "pair_gxi", "input_grad": "input_grad", "carry": "hidden_grad"}

# (n_nets, E, S, N, d0, d1, K, gate, noise, targets): N at the tile edges, K in {0, 1, S - 1}, targets in any order with a repeat
KERNEL_CASES_EMU = [
    (1, 2, 3, 2, 5, 8, 2, "through", True, (0, 1, 2)),
    (1, 1, 3, 3, 5, 8, 1, "held", True, (2, 0, 2)),
    (5, 1, 2, 3, 5, 8, 1, "through", True, (0, 1)),
    (1, 1, 2, 16, 5, 8, 1, "through", False, (1,)),
    (2, 1, 4, 17, 5, 8, 3, "through", True, (3, 1)),
    (1, 2, 3, 17, 5, 0, 0, "held", True, (0, 1, 2)),
    (1, 1, 2, 17, 64, 64, 1, "through", True, (1, 0)),
    (1, 1, 2, 33, 5, 8, 0, "through", True, (0, 1)),
    (1, 1, 3, 33, 5, 0, 2, "held", False, (2,)),
    (1, 1, 3, 33, 5, 8, 2, "through", True, (2, 1)),
]
KERNEL_CASES_GPU = [
    (1, 1, 3, 48, 5, 8, 2, "through", True, (2, 0)),
    (2, 1, 2, 49, 5, 0, 1, "through", False, (1,)),
    (1, 2, 2, 63, 5, 8, 1, "held", True, (1, 0)),
    (1, 1, 4, 64, 5, 8, 3, "through", True, (3, 2)),
    (1, 1, 2, 64, 64, 64, 0, "held", False, (0, 1)),
]


def kernel_case_id(c):
    n, E, S, N, d0, d1, K, gate, noise, targets = c
    return f"n{n}_E{E}_S{S}_N{N}_d{d0}+{d1}_K{K}_{gate}_{'noise' if noise else 'nonoise'}_t{''.join(map(str, targets))}"


def _zero_bits(t):
    return bool((_bits(t) == 0).all())


def carry_sq_host(carry):
    """sum_c carry[..., c]^2 as the plain fp32 loop: columns ascending, every product and sum rounded on its own"""
    c = carry.detach().cpu().float()
    s = torch.zeros(c.shape[:-1], dtype=torch.float32)
    for col in range(c.shape[-1]):
        p = c[..., col] * c[..., col]
        s = s + p
    return s


def run_trace(case, saved, S, v, targets, K, gate="through", want=TOUTS, out=None, scratch=None):
    res = dict(ops.gat_saliency_trace(case.arena, saved, S, v, list(targets), K, gate_through=gate == "through", want=want, out=out, scratch=scratch))
    _sync(case.device)
    res.pop("_keep")
    return res


def one_step_chain(case, saved, E, S, v, targets, K, gate):
    """the judge of check 1: lag by lag ``ops.gat_saliency`` over the whole record with the cotangent rows of the targets that reach
    a row (the others 0); two targets on one row go into launches of their own -> dict of [n, E, T, K+1, ...] + ``exists`` [T, K+1]"""
    n, T, N = v.shape[0], len(targets), v.shape[3]
    dev = v.device
    cot = v.clone()
    ref, exists = {}, torch.zeros(T, K + 1, dtype=torch.bool)
    for k in range(K + 1):
        todo = [t for t in range(T) if targets[t] - k >= 0]
        nxt = cot.clone()
        while todo:
            take, rows = [], set()
            for t in todo:
                if targets[t] - k not in rows:
                    rows.add(targets[t] - k)
                    take.append(t)
            todo = [t for t in todo if t not in take]
            vfull = torch.zeros(n, E, S, N, A, device=dev)
            for t in take:
                vfull[:, :, targets[t] - k] = cot[:, :, t]
            one = ops.gat_saliency(case.arena, saved, vfull.view(n, E * S, N, A), gate_through=gate == "through", want=SC.OUTS)
            _sync(case.device)
            for t in take:
                exists[t, k] = True
                for key, src in ONE_STEP.items():
                    row = one[src].unflatten(1, (E, S))[:, :, targets[t] - k]
                    if key not in ref:
                        ref[key] = torch.zeros(n, E, T, K + 1, *row.shape[2:], device=dev)
                    ref[key][:, :, t, k] = row
                nxt[:, :, t] = one["hidden_grad"].unflatten(1, (E, S))[:, :, targets[t] - k]
        cot = nxt
    return ref, exists


# ------------------------------------------------------------------------------------------------ 1: bit for bit against the one-step kernel
def check_kernel_bits(device, n, E, S, N, d0, d1, K, gate, noise, targets):
    case = SC.get_case((n, E * S, N, d0, d1), device, 7)
    _, saved = case.forward(0.25, noise)
    if gate == "held":
        saved["gru"].fill_(float("nan"))                                      # a held gate never reads the pair-GRU record
    T = len(targets)
    v = torch.randn(n, E, T, N, A, generator=torch.Generator().manual_seed(3 + N + K)).to(device)
    got = run_trace(case, saved, S, v, targets, K, gate)
    ref, exists = one_step_chain(case, saved, E, S, v, targets, K, gate)
    assert torch.equal(exists, torch.tensor([[k <= r for k in range(K + 1)] for r in targets]))
    for t in range(T):
        for k in range(K + 1):
            for key in TOUTS:
                slot = got[key][:, :, t, k]
                if not exists[t, k]:
                    assert _zero_bits(slot), (key, t, k, "the slot of a lag that does not exist is not +0.0")
                elif key == "carry_sq":
                    assert torch.equal(slot.cpu(), carry_sq_host(got["carry"][:, :, t, k])), (t, k, "carry_sq is not the fp32 host loop")
                else:
                    assert torch.isfinite(slot).all(), (key, t, k)
                    assert torch.equal(_bits(slot), _bits(ref[key][:, :, t, k])), (key, t, k, "bits differ from ops.gat_saliency's")
    assert got["grad"][:, :, 0, 0].abs().max() > 0
    return {}


# ------------------------------------------------------------------------------------------------ the method's inputs
def _policy(device, N, nA=2, **kw):
    return SC._policy(device, max_vehicle_num=N, n_agents=nA, **kw)


class Episode:
    """random inputs of the method for a policy: history in [-1, 1] with presence column 0 non-zero, behaviour latents on the simplex,
    a small hidden0, gumbel noise and a cotangent per (env, step)"""

    def __init__(self, args, E, S, seed=5):
        nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
        gen = torch.Generator().manual_seed(seed + 10 * N + S)
        self.hist = torch.rand(E, S, nA, N, d, generator=gen) * 2 - 1
        self.hist[..., 0] = 1.0
        self.lat = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
        self.h0 = torch.randn(E, nA, N, A, generator=gen) * 0.1
        self.noise = _gumbel(gen, nA, E, S, N, N - 1, 2)
        self.tgt = torch.randn(E, S, nA, N, A, generator=gen)
        self.dims = (E, S, nA, N, d, Z)

    def call(self, pol, device, **kw):
        to = lambda t: t.to(device) if torch.is_tensor(t) else t                 # noqa: E731
        kw = {k: to(v) for k, v in kw.items()}
        kw.setdefault("hidden0", to(self.h0))
        res = pol.attention_saliency_trace(to(self.hist), to(self.lat), **kw)
        _sync(device)
        return res


RESULT_KEYS = ("pair_gl1", "pair_gxi", "grad", "input_grad", "carry", "carry_l2")


def _same_slots(a, b, what, keys=RESULT_KEYS):
    for k in keys:
        if k in a and k in b:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


# ------------------------------------------------------------------------------------------------ 2: bit for bit against the public route
def by_hand(pol, ep, device, K, targets, target, noise, gate):
    """the route the one-step methods offer: ``attention_trace``, then per lag ONE ``attention_saliency`` call on the shifted slices
    of the targets the lag exists for, the carries as tensor targets -> (trace, dict of [E, T, K+1, ...] with zeros where no lag is)"""
    E, S, nA, N, d, Z = ep.dims
    to = lambda t: t.to(device)                                               # noqa: E731
    kw = dict(noise=to(ep.noise), deterministic=False) if noise else dict(deterministic=True)
    tr = pol.attention_trace(to(ep.hist), to(ep.lat), hidden0=to(ep.h0), want=(), _stats=False, **kw)
    hid = torch.cat([to(ep.h0)[:, None], tr["latent"][:, :-1]], 1)
    T = len(targets)
    out = {}
    cot = None
    for k in range(K + 1):
        live = [t for t in range(T) if targets[t] - k >= 0]
        if not live:
            break
        steps = [targets[t] - k for t in live]
        skw = dict(hidden=hid[:, steps], gate=gate, want=("pair", "grad"))
        if noise:
            skw.update(noise=to(ep.noise)[:, :, steps].contiguous(), deterministic=False)
        if k == 0:
            skw["target"] = to(ep.tgt)[:, targets] if target == "tensor" else target
        else:
            skw["target"] = cot[:, live].contiguous()
        one = pol.attention_saliency(to(ep.hist)[:, steps], to(ep.lat)[:, steps], **skw)
        _sync(device)
        if k == 0:
            out["target_vector"] = one["target_vector"].clone()
            cot = torch.zeros(E, T, nA, N, A, device=device)
        for key, src in ONE_STEP.items():
            if key not in out:
                out[key] = torch.zeros(E, T, K + 1, *one[src].shape[2:], device=device)
            out[key][:, live, k] = one[src]
        for key in ("active_h", "active_v"):
            out.setdefault(key, {})
            for pos, s in enumerate(steps):
                out[key][s] = one[key][:, pos]
        cot[:, live] = one["hidden_grad"]
    return tr, out


def check_public_route(device, N=5, E=1, S=4, K=2, targets=None, target="tensor", noise=False, gate="through"):
    args, pol, _ = _policy(device, N)
    ep = Episode(args, E, S)
    tg = list(range(S)) if targets is None else list(targets)
    kw = dict(lags=K, targets=targets, gate=gate, want=("pair", "grad", "carry"))
    kw["target"] = ep.tgt[:, tg] if target == "tensor" else target
    if noise:
        kw.update(noise=ep.noise, deterministic=False)
    got = ep.call(pol, device, **kw)
    tr, ref = by_hand(pol, ep, device, K, tg, target, noise, gate)
    assert torch.equal(_bits(got["latent"]), _bits(tr["latent"])), "latent != attention_trace's"
    assert torch.equal(_bits(got["target_vector"]), _bits(ref["target_vector"])), "target_vector"
    for key in ONE_STEP:
        assert torch.equal(_bits(got[key]), _bits(ref[key])), (key, "differs from the by-hand route")
    # (torch's sqrt where the method takes it: the device's and the host's differ in the last bit)
    assert torch.equal(got["carry_l2"], torch.sqrt(carry_sq_host(ref["carry"]).to(device))), "carry_l2"
    for key in ("active_h", "active_v"):
        for s, rows in ref[key].items():
            assert torch.equal(got[key][:, s], rows), (key, s)
    assert got["targets"].tolist() == tg
    assert torch.equal(got["lag_valid"], torch.tensor([[k <= s for k in range(K + 1)] for s in tg]))
    return {}


# ------------------------------------------------------------------------------------------------ 3: against fp64
def reference_chain(p, obs, h_start, noise, v, tau, ah, av, held, dtype):
    """one (net, env, target): the L steps the lags reach, oldest first -- obs [L, N, D], h_start [N, A] (the state entering the
    oldest step), noise [L, N, N-1, 2], v [N, A], ah / av [L, N, 32] bool -> latent [N, A] of the target step, grad [L, N, N, D]
    (d y_i / d obs of each step), carry [L, N, A] (d y_i / d the state entering each step) in ``dtype``"""
    n_steps, N = obs.shape[:2]
    p = {k: t.to(dtype) for k, t in p.items()}
    rep = lambda t: t.to(dtype)[None].expand(N, *t.shape).clone()                 # noqa: E731
    obs_r = [rep(obs[s]).requires_grad_(True) for s in range(n_steps)]
    h = rep(h_start).requires_grad_(True)
    states = []
    for s in range(n_steps):
        states.append(h)
        with SC._pinned(ah[s][None].expand(N, N, A), av[s][None].expand(N, N, A), held):
            h = O.gat_forward(p, obs_r[s], h.reshape(N * N, A), rep(noise[s]).reshape(-1, 2), tau=tau).view(N, N, A)
    idx = torch.arange(N)
    y = (v.to(dtype) * h[idx, idx]).sum()
    grads = torch.autograd.grad(y, obs_r + states)
    return dict(latent=h[0].detach(), grad=torch.stack(grads[:n_steps]), carry=torch.stack([g[idx, idx] for g in grads[n_steps:]]))


def method_reference(gat, ep, got, K, targets, tau, gate, noise, dtype):
    """every (env, target, agent) of the method's result through the judge: dict of [E, T, K+1, nA, ...], zeros where no lag is"""
    E, S, nA, N, d, Z = ep.dims
    D = d + Z
    obs = torch.cat([ep.hist, ep.lat], -1)
    T = len(targets)
    cpu = {k: torch.as_tensor(got[k]).cpu() for k in ("target_vector", "active_h", "active_v", "latent")}
    out = dict(grad=torch.zeros(E, T, K + 1, nA, N, N, D, dtype=dtype), carry=torch.zeros(E, T, K + 1, nA, N, A, dtype=dtype),
               latent=torch.zeros(E, T, nA, N, A, dtype=dtype))
    xs = torch.zeros(E, T, K + 1, nA, N, D, dtype=dtype)                            # the inputs of step s - k, for pair_gxi
    for e in range(E):
        for t, s in enumerate(targets):
            lo = max(0, s - K)
            for i in range(nA):
                start = ep.h0[e, i] if lo == 0 else cpu["latent"][e, lo - 1, i]      # (the kernel's own latent: 1e-7 from the judge's)
                nz = ep.noise[i, e, lo:s + 1] if noise else torch.zeros(s + 1 - lo, N, N - 1, 2)
                r = reference_chain(gat[i], obs[e, lo:s + 1, i], start, nz, cpu["target_vector"][e, t, i], tau, cpu["active_h"][e, lo:s + 1, i],
                                    cpu["active_v"][e, lo:s + 1, i], gate == "held", dtype)
                out["latent"][e, t, i] = r["latent"]
                for k in range(s - lo + 1):
                    out["grad"][e, t, k, i] = r["grad"][s - lo - k]
                    out["carry"][e, t, k, i] = r["carry"][s - lo - k]
                    xs[e, t, k, i] = obs[e, s - k, i].to(dtype)
    out.update(SC.derived(out["grad"], xs, d))
    return out


FP64_CASES = [(2, 1, 1.0), (5, 2, 0.25), (17, 3, 0.01), (33, 1, 0.01), (5, 3, 0.01), (17, 1, 1.0), (33, 2, 0.25), (2, 3, 0.01)]    # (N, K, tau)


def check_fp64(device, N, K, tau, E=1, gate="through", noise=False):
    """targets: the last step (every lag exists) and step K - 1 (the last lag does not), S = K + 1"""
    args, pol, gat = _policy(device, N, nA=2 if N < 33 else 1)
    S = K + 1
    ep = Episode(args, E, S, seed=9)
    targets = [K - 1, K]
    kw = dict(lags=K, targets=targets, target=ep.tgt[:, targets], gate=gate, tau=tau, want=("pair", "grad", "carry"))
    if noise:
        kw.update(noise=ep.noise, deterministic=False)
    got = ep.call(pol, device, **kw)
    r64 = method_reference(gat, ep, got, K, targets, tau, gate, noise, torch.float64)
    r32 = method_reference(gat, ep, got, K, targets, tau, gate, noise, torch.float32)
    worst = {}
    for k in range(K + 1):
        for key in ("grad", "pair_gl1", "pair_gxi", "input_grad", "carry"):
            ref = r64[key][:, :, k]
            e32, err = _grad_err(r32[key][:, :, k], ref), _grad_err(got[key][:, :, k], ref)
            print("N", N, "K", K, "tau", tau, gate, "lag", k, key, "err", err, "e32", e32, "max|ref|", ref.abs().max().item())
            _worse(worst, f"{key}_tau{tau}", err)
            _worse(worst, f"{key}_tau{tau}_e32", e32)
            assert e32 <= E32_CAP, (key, k, "the fp32 oracle itself is off by", e32)
            assert err <= max(TOL, E32_FACTOR * e32), (key, "lag", k, err, e32)
    err = _grad_err(got["latent"][:, targets], r64["latent"])
    e32 = _grad_err(r32["latent"], r64["latent"])
    _worse(worst, f"latent_tau{tau}", err)
    _worse(worst, f"latent_tau{tau}_e32", e32)
    assert e32 <= E32_CAP, ("latent", "the fp32 oracle itself is off by", e32)
    assert err <= max(TOL, E32_FACTOR * e32), ("latent", err, e32)
    return worst


# ------------------------------------------------------------------------------------------------ 4: exact statements
def _halving_sum_numpy(x, axis):
    """the method's stated order: the axis zero-padded to a power of two, its upper half added to its lower half until one is left"""
    n, size = x.shape[axis], 1
    while size < n:
        size *= 2
    if size > n:
        pad = list(x.shape)
        pad[axis] = size - n
        x = np.concatenate([x, np.zeros(pad, dtype=x.dtype)], axis=axis)
    while size > 1:
        size //= 2
        x = np.take(x, range(size), axis=axis) + np.take(x, range(size, 2 * size), axis=axis)
    return np.squeeze(x, axis=axis)


def lag_l1_numpy(pair_gl1, hist, targets, K, presence_col):
    """the float64 restatement of lag_l1 / lag_pairs: pair_gl1 [E,T,K+1,nA,N,N,n_src], hist [E,S,nA,N,d] numpy.  Which pairs count is
    decided here entry by entry; the counting entries of an environment are summed in the order the method states -- entities, then
    egos, then targets, each axis by pairwise halving -- and the environments are added in order."""
    E, T, _, nA, N, _, n_src = pair_gl1.shape
    tot, cnt = np.zeros((nA, K + 1, n_src, 2)), np.zeros((nA, K + 1, 2))
    for e in range(E):
        g = np.zeros((2, nA, T, K + 1, N, N, n_src))                            # [i == j] first: the counting entries, 0.0 elsewhere
        for t, s in enumerate(targets):
            for k in range(min(K, s) + 1):
                for a in range(nA):
                    for i in range(N):
                        for j in range(N):
                            if presence_col >= 0 and (hist[e, s, a, i, presence_col] == 0 or hist[e, s - k, a, j, presence_col] == 0):
                                continue
                            g[int(i == j), a, t, k, i, j] = pair_gl1[e, t, k, a, i, j].astype(np.float64)
                            cnt[a, k, int(i == j)] += 1
        for diag in range(2):
            tot[..., diag] += _halving_sum_numpy(_halving_sum_numpy(_halving_sum_numpy(g[diag], 4), 3), 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cnt[:, :, None, :] > 0, tot / cnt[:, :, None, :], np.nan), cnt


def check_exact(device, N=3, E=2, S=4, K=3):
    args, pol, gat = _policy(device, N)
    ep = Episode(args, E, S, seed=2)
    ep.hist[0, 1:3, :, 2, 0] = 0.0                                             # a planted absent vehicle: entity 2, steps 1 and 2, env 0
    ep.hist[1, 3, 0, 1, 0] = 0.0                                               # ... and an absent ego at a target step
    tgt = ep.tgt.clone()
    tgt[:, :, :, 0] = 0.0                                                      # ego 0: a zero cotangent
    full = ep.call(pol, device, lags=K, target=tgt, tau=0.25, want=("pair", "grad", "carry"))
    valid = full["lag_valid"]
    assert torch.equal(valid, torch.tensor([[k <= s for k in range(K + 1)] for s in range(S)])) and not valid.all()
    for key in RESULT_KEYS:
        for t in range(S):
            for k in range(K + 1):
                if not valid[t, k]:
                    assert _zero_bits(full[key][:, t, k]), (key, t, k, "the slot of a lag that does not exist is not +0.0")
                else:
                    assert full[key][:, t, k].abs().max() > 0, (key, t, k)
    for key in ("grad", "pair_gl1", "pair_gxi", "carry", "carry_l2"):             # a zero cotangent: exact zeros at every lag
        row = full[key][:, :, :, :, 0].cpu()
        assert torch.equal(row, torch.zeros_like(row)), (key, "of an ego with v = 0 is not exactly 0")
    assert torch.equal(full["carry_l2"], torch.sqrt(carry_sq_host(full["carry"]).to(device))), "carry_l2 is not torch's sqrt of the fp32 host loop"
    # lag_l1 / lag_pairs against the numpy restatement -- with the default presence column, with none, and with a target at step 0 alone
    worst = {}
    for pc, targets in ((0, None), (-1, None), (0, [0])):
        res = full if (pc == 0 and targets is None) else ep.call(pol, device, lags=K, target=tgt[:, targets] if targets else tgt, tau=0.25,
                                                                    targets=targets, presence_col=pc)
        tl = list(range(S)) if targets is None else targets
        ref, cnt = lag_l1_numpy(res["pair_gl1"].cpu().numpy(), ep.hist.numpy(), tl, K, pc)
        assert res["lag_l1"].dtype == np.float64 and res["lag_l1"].shape == (args.n_agents, K + 1, 2, 2)
        assert np.array_equal(res["lag_pairs"], cnt), (pc, targets)
        assert np.array_equal(res["lag_l1"], ref, equal_nan=True), (pc, targets, "lag_l1 is not the float64 restatement")
        if targets == [0]:
            assert np.isnan(res["lag_l1"][:, 1:]).all() and np.isfinite(res["lag_l1"][:, 0]).all()
    pairs = full["lag_pairs"]
    assert pairs[0, 0, 0] < E * S * N * (N - 1) and pairs[0, 0, 0] > 0, "the planted absent vehicle does not show in the counts"
    return worst


def check_linearity(device, N=17, K=2, tau=1.0, alpha=0.75, beta=-1.5):
    """Linearity in the cotangent at every lag, as attention_saliency_checks.check_linearity states it for one step, with its bound:
    E32_FACTOR x the one-step fp32 oracle's own residual for the same statement on the same row.  Lag k of a run is the one-step map
    of step s - k applied to that run's cotangent c^(k-1) (v itself at lag 0).  So with cv = c^(k-1)(v), cw = c^(k-1)(w) and their
    fp32 combination mix = alpha cv + beta cw, the kernel's lag-k slots G(cv), G(cw) and a launch of the same kernel on step s - k
    with mix as its cotangent must satisfy G(mix) = alpha G(cv) + beta G(cw) as far as the fp32 oracle of that one step does."""
    args, pol, gat = _policy(device, N, nA=1)
    S = K + 1
    ep = Episode(args, 1, S, seed=3)
    w = torch.randn(1, 1, 1, N, A, generator=torch.Generator().manual_seed(5))
    v = ep.tgt[:, K:K + 1]
    runs = {name: ep.call(pol, device, lags=K, targets=[K], target=t, tau=tau, want=("grad", "carry")) for name, t in (("v", v), ("w", w))}
    obs = torch.cat([ep.hist, ep.lat], -1)
    ah, av, latent = runs["v"]["active_h"].cpu(), runs["v"]["active_v"].cpu(), runs["v"]["latent"].cpu()
    worst = {}

    def lin_err(G):
        return _grad_err(alpha * G["v"] + beta * G["w"], G["mix"])                # the fp32 rounding of the sum is part of the statement

    for k in range(K + 1):
        s = K - k
        cot = {name: (t if k == 0 else runs[name]["carry"][:, :, k - 1].cpu()) for name, t in (("v", v), ("w", w))}      # [1, 1, 1, N, A]
        cot["mix"] = alpha * cot["v"] + beta * cot["w"]
        G = {name: runs[name]["grad"][0, 0, k, 0].cpu() for name in ("v", "w")}
        G["mix"] = ep.call(pol, device, lags=0, targets=[s], target=cot["mix"], tau=tau, want=("grad",))["grad"][0, 0, 0, 0].cpu()
        start = ep.h0[0, 0] if s == 0 else latent[0, s - 1, 0]
        o32 = {name: SC.reference_scene(gat[0], obs[0, s, 0], start, torch.zeros(N, N - 1, 2), c[0, 0, 0], tau, ah[0, s, 0], av[0, s, 0], False,
                                        torch.float32)["grad"] for name, c in cot.items()}
        e_oracle, e_kernel = lin_err(o32), lin_err(G)
        print("linearity lag", k, "kernel", e_kernel, "fp32 oracle", e_oracle)
        _worse(worst, f"linearity_lag{k}", e_kernel)
        _worse(worst, f"linearity_lag{k}_e32", e_oracle)
        assert e_oracle > 0
        assert e_kernel <= E32_FACTOR * e_oracle, (k, e_kernel, e_oracle)
    return worst


# ------------------------------------------------------------------------------------------------ 5: independence
def check_independence(device, N=3, E=2, S=4, K=2):
    args, pol, _ = _policy(device, N)
    ep = Episode(args, E, S, seed=4)
    want = ("pair", "grad", "carry")
    base = dict(lags=K, target=ep.tgt, tau=0.25, noise=ep.noise, deterministic=False, want=want)
    full = ep.call(pol, device, **base)
    # the other targets / the targets list
    for tl in ([1, 3], [0, 2, 3]):
        sub = ep.call(pol, device, **dict(base, targets=tl, target=ep.tgt[:, tl]))
        _same_slots(sub, {k: full[k][:, tl] for k in RESULT_KEYS}, f"targets={tl}")
        assert torch.equal(_bits(sub["latent"]), _bits(full["latent"]))
    # K: a shorter lags gives a prefix along the lag axis
    for K2 in (1,):
        short = ep.call(pol, device, **dict(base, lags=K2))
        _same_slots(short, {k: full[k][:, :, :K2 + 1] for k in RESULT_KEYS}, f"lags={K2}")
    # the outputs asked for
    few = ep.call(pol, device, **dict(base, want=()))
    assert set(few) == set(full) - {"pair_gl1", "pair_gxi", "grad", "carry", "lag_l1", "lag_pairs"}, set(few) ^ set(full)
    _same_slots(few, full, "want=()")
    # the other scenes: an environment alone, and the environments at other positions
    e1 = Episode(args, E, S, seed=4)
    for name in ("hist", "lat", "h0", "tgt"):
        setattr(e1, name, getattr(ep, name)[1:2])
    e1.noise = ep.noise[:, 1:2]
    e1.dims = (1,) + ep.dims[1:]
    alone = e1.call(pol, device, **dict(base, target=e1.tgt, noise=e1.noise))
    _same_slots(alone, {k: full[k][1:2] for k in RESULT_KEYS}, "an environment alone")
    rev = Episode(args, E, S, seed=4)
    for name in ("hist", "lat", "h0", "tgt"):
        setattr(rev, name, getattr(ep, name).flip(0).contiguous())
    rev.noise = ep.noise.flip(1).contiguous()
    flipped = rev.call(pol, device, **dict(base, target=rev.tgt, noise=rev.noise))
    _same_slots(flipped, {k: full[k].flip(0) for k in RESULT_KEYS}, "environments at other positions")
    # the chunking: just above the refusal threshold -> one environment per chunk and several runs of targets
    try:
        ep.call(pol, device, **dict(base, max_workspace_mb=1e-6))
        raise AssertionError("a workspace of one byte was accepted")
    except ValueError as err:
        need = float(re.search(r"\(([0-9.]+) MB\)", str(err)).group(1))
    calls = {"walk": 0, "trace": 0}
    real_walk, real_trace = ops.gat_trace, ops.gat_saliency_trace

    def walk(*a, **k):
        calls["walk"] += 1
        return real_walk(*a, **k)

    def trace(*a, **k):
        calls["trace"] += 1
        return real_trace(*a, **k)

    with mock.patch.object(ops, "gat_trace", walk), mock.patch.object(ops, "gat_saliency_trace", trace):
        small = ep.call(pol, device, **dict(base, max_workspace_mb=need + 0.06))
    assert calls["walk"] == E and calls["trace"] >= 2 * E, (calls, "the chunked call did not split into environments and runs of targets")
    _same_slots(small, full, "chunked")
    for k in ("latent", "target_vector", "active_h", "active_v"):
        assert torch.equal(_bits(small[k]), _bits(full[k])), (k, "chunked")
    assert np.array_equal(small["lag_l1"], full["lag_l1"], equal_nan=True) and np.array_equal(small["lag_pairs"], full["lag_pairs"]), \
        "lag_l1 depends on the chunking"
    with mock.patch.object(ops, "gat_trace", walk), mock.patch.object(ops, "gat_saliency_trace", trace):
        calls.update(walk=0, trace=0)
        ep.call(pol, device, **base)
    assert calls == {"walk": 1, "trace": 1}, (calls, "the default workspace holds this case in one chunk")
    return {}


# ------------------------------------------------------------------------------------------------ 6: ownership
def check_ownership(device, n=1, E=2, S=2, N=17, K=1, tau=0.25):
    case = SC.get_case((n, E * S, N, 5, 8), device, 4)
    _, saved = case.forward(tau)
    targets = (1, 0)
    T, D, n_src = len(targets), 13, 2
    v = torch.randn(n, E, T, N, A, generator=torch.Generator().manual_seed(8)).to(device)
    ref = run_trace(case, saved, S, v, targets, K)
    shapes = {"grad": (N, N, D), "pair_gl1": (N, N, n_src), "pair_gxi": (N, N, n_src), "input_grad": (N, D), "carry": (N, A), "carry_sq": (N,)}

    def carve(k, shift=0.0):
        inner = int(np.prod(shapes[k]))
        pad = 7 if k.startswith("pair") else 5                                # the two pair maps share their strides
        slots = n * E * T * (K + 1)
        total = slots * (inner + pad) + 64
        sent = _sentinel(total) + shift
        sent[:4] = float("nan")
        sent[-4:] = float("nan")
        buf = sent.clone().to(device)
        view = buf[32:32 + slots * (inner + pad)].view(n, E, T, K + 1, inner + pad)[..., :inner].unflatten(-1, shapes[k])
        mask = torch.ones(total, dtype=torch.bool)
        mask[32:32 + slots * (inner + pad)].view(n, E, T, K + 1, inner + pad)[..., :inner] = False
        return sent, buf, view, mask

    for wanted in (("input_grad", "carry_sq"), ("pair_gl1", "pair_gxi")):
        bufs = {k: carve(k) for k in shapes}
        got = run_trace(case, saved, S, v, targets, K, want=wanted, out={k: bufs[k][2] for k in wanted})
        for k, (sent, buf, view, mask) in bufs.items():
            host = buf.cpu()
            if k not in wanted:
                assert torch.equal(host.view(torch.int32), sent.view(torch.int32)), (k, "was not asked for and was written")
                continue
            assert got[k].data_ptr() == view.data_ptr()
            assert torch.equal(_bits(view), _bits(ref[k])), (k, "differs inside a padded buffer")
            assert torch.equal(host[mask].view(torch.int32), sent[mask].view(torch.int32)), (k, "a float outside the owned views was written")
    b2 = {k: carve(k, 0.25) for k in shapes}                                  # every owned float is written, the slots of no lag too
    run_trace(case, saved, S, v, targets, K, out={k: b2[k][2] for k in shapes})
    for k in shapes:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (k, "an owned float was left unwritten")
    # a used scratch, again and again: the same bits
    scratch = torch.full((ops.gat_saliency_trace_scratch_floats(n, E, T, N) + 16,), float("nan"), device=device)
    for _ in range(2):
        again = run_trace(case, saved, S, v, targets, K, scratch=scratch)
        for k in TOUTS:
            assert torch.equal(_bits(again[k]), _bits(ref[k])), (k, "depends on what the scratch held")
    assert torch.isnan(scratch[-16:]).all(), "floats behind the needed scratch were written"
    # NaN around the operands: the guard floats of the source buffers, and v as a strided view into a NaN-filled buffer
    keep0, keep1 = case.buf0.clone(), case.buf1.clone()
    try:
        for buf, lead, d in ((case.buf0, 2, 5), (case.buf1, 1, 8)):
            buf[:, :, :lead] = float("nan")
            buf[:, :, lead + N * d:] = float("nan")
        case.upload()
        _, saved2 = case.forward(tau)
        vbuf = torch.full((n, E, T, N * A + 8), float("nan"), device=device)
        vv = vbuf[..., 4:4 + N * A].unflatten(-1, (N, A))
        vv.copy_(v)
        nan_around = run_trace(case, saved2, S, vv, targets, K)
        for k in TOUTS:
            assert torch.equal(_bits(nan_around[k]), _bits(ref[k])), (k, "NaN around the inputs")
    finally:
        case.buf0.copy_(keep0)
        case.buf1.copy_(keep1)
        case.upload()
    return {}


# ------------------------------------------------------------------------------------------------ 7: the chain with the policy
def check_chain(device, dims=(2, 1, 3, 3, 5), tau=0.25):
    """d sum_s log pi(a*_s) / d [history_u || behavior_latent_u] in total = the policy's own hist / beh columns at u + sum_k
    input_grad[target u + k, lag k] of this method seeded with the policy's att columns, against autograd through the GAT CHAIN from
    hidden0 -> build_inputs_train -> actor_evaluate with the recorded actor GRU state (attention_saliency_checks.check_chain with
    the attention state no longer held)"""
    from iplan_amd import synth
    from iplan_amd.nova.prediction_policy import Prediction_policy
    from tests import saliency_checks as PS
    from tests.oracle_checks import _Log
    from tests.policy_trace_checks import _params
    nA, E, S, N, d = dims
    case = PS.Case(dims, device, seed=3, avail_ones=True)                        # (every action available: no step whose log pi is the constant 0)
    a, f = case.args, dict(case.f)
    Z, M, K = a.latent_dim, a.rnn_hidden_dim, S - 1
    torch.manual_seed(23)
    pol = Prediction_policy(a, _Log())
    gat = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in pol.pred_GAT]
    gen = torch.Generator().manual_seed(8)
    hist = torch.rand(E, S, nA, N, d, generator=gen) * 2 - 1
    beh = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
    h0 = torch.randn(E, nA, N, A, generator=gen) * 0.1
    call = lambda **kw: pol.attention_saliency_trace(hist.to(device), beh.to(device), hidden0=h0.to(device), lags=K, tau=tau, want=(), **kw)   # noqa: E731
    first = call()
    f["history"] = torch.cat([hist, f["history"][:, S:]], 1)                   # the policy sees exactly this latent as its att columns
    f["behavior_latent"] = torch.cat([beh, f["behavior_latent"][:, S:]], 1)
    f["attention_latent"] = torch.cat([first["latent"].cpu(), f["attention_latent"][:, S:]], 1)
    batch = synth.DictBatch(f, E, S + 1).to(device)
    sal = case.mac.saliency(batch, target="recorded", which="actor", want=("input_grad", "act"), steps=slice(0, S))
    W = d + A + Z
    ent = sal["actor_input_grad"][..., :N * W].reshape(E, S, nA, N, W)
    res = call(target=ent[..., d:d + A].contiguous())
    _sync(device)
    assert torch.equal(_bits(res["latent"]), _bits(first["latent"]))
    ig = res["input_grad"].cpu()                                               # [E, T = S, K+1, nA, N, d+Z]
    total = torch.cat([ent[..., :d], ent[..., d + A:]], -1).cpu().clone()
    through_time = torch.zeros_like(total)
    for u in range(S):
        for k in range(S - u):
            total[:, u] += ig[:, u + k, k]
            if k:
                through_time[:, u] += ig[:, u + k, k]
    ah, av = res["active_h"].cpu(), res["active_v"].cpu()
    n_act = a.n_actions
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ap, _ = _params(case.mac, dtype)
        ref = torch.zeros(E, S, nA, N, d + Z, dtype=dtype)
        for i in range(nA):
            h_leaf = hist[:, :, i].to(dtype).clone().requires_grad_(True)
            b_leaf = beh[:, :, i].to(dtype).clone().requires_grad_(True)
            p = {k: t.to(dtype) for k, t in gat[i].items()}
            state, atts = h0[:, i].to(dtype).reshape(E * N, A), []
            for s in range(S):
                with SC._pinned(ah[:, s, i], av[:, s, i], False):
                    state = O.gat_forward(p, torch.cat([h_leaf[:, s], b_leaf[:, s]], -1), state, torch.zeros(E * N * (N - 1), 2, dtype=dtype), tau=tau)
                atts.append(state.view(E, N, A))
            x = O.build_inputs_train(i, h_leaf, torch.stack(atts, 1), b_leaf, torch.zeros(E, S, n_act, dtype=dtype), nA, a.GAT_enable,
                                     a.Behavior_enable)
            acts = f["actions"][:, :S, i, 0]
            last = torch.cat([torch.full_like(acts[:, :1], -1), acts[:, :-1]], 1)
            oh = torch.zeros(E, S, n_act, dtype=dtype)
            oh.scatter_(-1, last.clamp_min(0).unsqueeze(-1), (last >= 0).to(dtype).unsqueeze(-1))
            idoh = torch.zeros(E, S, nA, dtype=dtype)
            idoh[..., i] = 1
            x = torch.cat([x[..., :x.shape[-1] - n_act - nA], oh, idoh], -1).reshape(E * S, -1)
            hints = (sal["actor_act1"][:, :, i].reshape(E * S, M).cpu() > 0, sal["actor_act2"][:, :, i].reshape(E * S, M).cpu() > 0)
            logp, _ = O.actor_evaluate(ap[i], x, f["rnn_states_actors"][:, :S, i].reshape(E * S, M).to(dtype), acts.reshape(-1),
                                       f["avail_actions"][:, :S, i].reshape(E * S, -1), relu_hint=hints, use_relu=a.use_ReLU)
            gh, gb = torch.autograd.grad(logp.sum(), (h_leaf, b_leaf))
            ref[:, :, i] = torch.cat([gh, gb], -1)
        refs[dtype] = ref
    r64 = refs[torch.float64]
    worst = {}
    for u in range(S):                                                         # every step on its own
        e32, err = _grad_err(refs[torch.float32][:, u], r64[:, u]), _grad_err(total[:, u], r64[:, u])
        print("chain: step", u, "err", err, "e32", e32, "share through time", through_time[:, u].abs().max().item() / max(r64[:, u].abs().max().item(), 1e-30))
        _worse(worst, "chain", err)
        _worse(worst, "chain_e32", e32)
        assert e32 <= E32_CAP, (u, e32)
        assert err <= max(TOL, E32_FACTOR * e32), (u, err, e32)
    assert through_time[:, 0].abs().max() > 0 and ig[:, S - 1, S - 1].abs().max() > 0, "nothing went through time"
    assert all(r64[:, u].abs().max() > 0 for u in range(S))
    return worst


# ------------------------------------------------------------------------------------------------ 8: touches nothing, refusals
def check_touches_nothing(device, E=2):
    from iplan_amd import synth
    from iplan_amd.nova.prediction_policy import Prediction_policy
    from tests.oracle_checks import _Log
    args, pol, _ = SC._policy(device)
    nA, N, P, S = args.n_agents, args.max_vehicle_num, args.pred_length, args.pred_batch_size
    batch = synth.make_batch(args, E, seed=9, terminated_p=0.1, device=device)
    D = batch.data
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), ggrad=pol.gat_arena.grad.clone(), dgrad=pol.dec_arena.grad.clone(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer], rng=torch.get_rng_state(),
                  crng=torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, vars=sorted(vars(pol)))
    res = pol.attention_saliency_trace(D["history"][:, 1:5], D["behavior_latent"][:, :4], hidden0=D["attention_latent"][:, 0], lags=2,
                                       want=("pair", "grad", "carry"))
    _sync(device)
    assert torch.isfinite(res["grad"]).all()
    assert torch.equal(pol.gat_arena.data, before["gat"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert torch.equal(_bits(pol.gat_arena.grad), _bits(before["ggrad"])) and torch.equal(_bits(pol.dec_arena.grad), _bits(before["dgrad"]))
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"] and sorted(vars(pol)) == before["vars"]
    assert torch.equal(torch.get_rng_state(), before["rng"])
    if before["crng"] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), before["crng"])
    # numpy in -> numpy out (float64 histories, as the runner hands them over), the same numbers
    as_np = pol.attention_saliency_trace(D["history"][:, 1:5].double().cpu().numpy(), D["behavior_latent"][:, :4].cpu().numpy(),
                                         hidden0=D["attention_latent"][:, 0].cpu().numpy(), lags=2, want=("pair", "grad", "carry"))
    assert set(as_np) == set(res)
    for k, t in res.items():
        assert isinstance(as_np[k], np.ndarray) and np.array_equal(as_np[k], t.cpu().numpy() if torch.is_tensor(t) else t, equal_nan=True), k
    # a following learn() gives the same bits with and without a preceding call
    gen = torch.Generator().manual_seed(21)
    avail = args.episode_limit - P - 1
    sel = torch.stack([torch.randperm(E * avail, generator=gen)[:S] for _ in range(nA)]).numpy()
    noise = _gumbel(gen, nA, S, N, N - 1, 2).to(device)
    keep = (torch.rand(nA, P, S * N, args.attention_dim, generator=gen) < 1.0 - args.decoder_dropout).float().to(device)
    results = []
    for with_call in (False, True):
        torch.manual_seed(31)
        np.random.seed(32)
        p2 = Prediction_policy(args, _Log())
        if with_call:
            p2.attention_saliency_trace(D["history"][:, 1:4], D["behavior_latent"][:, :3], hidden0=D["attention_latent"][:, 0], lags=1, gate="held")
        losses = p2.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), p2.gat_arena.data.clone(), p2.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


def check_entry_point_refusals(device):
    """each of these is refused with its code and its own message, without a launch"""
    E, S, N, K = 1, 3, 5, 2
    case = SC.get_case((1, E * S, N, 5, 8), device, 6)
    _, saved = case.forward(1.0)
    targets = (2, 1)
    v = torch.randn(1, E, len(targets), N, A, generator=torch.Generator().manual_seed(2)).to(device)
    good = run_trace(case, saved, S, v, targets, K)
    lib = ops._lib(None)
    a, res, keep = ops.gat_saliency_trace_args(case.arena, saved, S, v, list(targets), K, True, TOUTS)
    t_host = keep[2]
    EINVAL, EALIGN = SC._codes()

    def get(obj, path):
        for name in path.split(".")[:-1]:
            obj = getattr(obj, name)
        return obj, path.split(".")[-1]

    def refused(code, text, **fields):
        fields = {k.replace("__", "."): v for k, v in fields.items()}
        old = {}
        for k, val in fields.items():
            o, name = get(a, k)
            old[k] = getattr(o, name)
            setattr(o, name, val)
        rc = lib.c.iplan_gat_saliency_trace(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, val in old.items():
            o, name = get(a, k)
            setattr(o, name, val)
        assert rc == code and msg.startswith("iplan_gat_saliency_trace:") and text in msg, (fields, rc, msg)

    assert lib.c.iplan_gat_saliency_trace(None, L.C.c_void_p(0)) == EINVAL and "null args" in lib.c.iplan_last_error().decode()
    refused(EINVAL, "N=1 outside", fwd__N=1)
    refused(EINVAL, "N=65 outside", fwd__N=65)
    refused(EINVAL, "bad dims", fwd__n_nets=0)
    refused(EINVAL, "bad dims", B=0)
    refused(EINVAL, "bad dims", R=0)
    refused(EINVAL, "bad dims", fwd__d0=0)
    refused(EINVAL, "bad dims", fwd__d1=-1)
    refused(EINVAL, "rows per net", R=S + 1)
    refused(EINVAL, "rows per net", fwd__B=E * S + 1)
    refused(EINVAL, "at least one target", T=0)
    refused(EINVAL, "K=-1 is negative", K=-1)
    refused(EINVAL, "gate_through=2", gate_through=2)
    refused(EINVAL, "did not save", fwd__saved__cell=None)
    refused(EINVAL, "did not save", fwd__saved__gru=None)
    refused(EINVAL, "null tensor pointer", v=None)
    refused(EINVAL, "null tensor pointer", fwd__src1=None)
    refused(EINVAL, "null tensor pointer", fwd__h_prev=None)
    refused(EINVAL, "target list is missing", targets=None)
    refused(EINVAL, "target list is missing", targets_host=None)
    for bad in (S, -1):
        t_host[1] = bad
        refused(EINVAL, "outside the record window")
        t_host[1] = targets[1]
    refused(EINVAL, "no output asked for", grad=None, pair_gl1=None, pair_gxi=None, input_grad=None, carry=None, carry_sq=None)
    refused(EINVAL, "must be positive", fwd__tau=0.0)
    refused(EINVAL, "are needed", scratch=None)
    refused(EINVAL, "are needed", scratch_floats=a.scratch_floats - 1)
    refused(EALIGN, "16-byte aligned", scratch=a.scratch + 4)
    lib.call("iplan_gat_saliency_trace", a, L.current_stream(device))           # the restored descriptor is accepted
    _sync(device)
    for k in TOUTS:
        assert torch.equal(_bits(res[k]), _bits(good[k])), (k, "after the refusals")
    # a held gate needs neither the pair-GRU record nor the scratch
    a.gate_through, a.scratch, a.scratch_floats = 0, None, 0
    a.fwd.saved.gru = None
    lib.call("iplan_gat_saliency_trace", a, L.current_stream(device))
    _sync(device)
    held = run_trace(case, saved, S, v, targets, K, gate="held")
    for k in TOUTS:
        assert torch.equal(_bits(res[k]), _bits(held[k])), (k, "held gate without record and scratch")
    del keep
    return {}


def check_method_refusals(device):
    args, pol, _ = SC._policy(device)
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    E, S = 1, 3
    hist, lat = torch.rand(E, S, nA, N, d).to(device), torch.rand(E, S, nA, N, Z).to(device)

    def refused(*a, **kw):
        try:
            pol.attention_saliency_trace(*a, **kw)
        except ValueError as e:
            assert "attention_saliency_trace" in str(e), e
            return str(e)
        raise AssertionError(f"not refused: {kw}")

    refused(hist)                                                             # behavior_latent missing
    refused(hist[0], lat)
    refused(hist[..., :d - 1], lat)
    refused(hist, lat[..., :Z - 1])
    refused(hist, lat, hidden0=torch.zeros(E, nA, N, A - 1))
    refused(hist, lat, hidden0=torch.zeros(E, S, nA, N, A))
    for lags in (-1, S, 1.0, True, "1"):
        refused(hist, lat, lags=lags)
    for targets in ([], [S], [-1], [1, 1], [2, 1], [0.5], [True], (t for t in [2, 1])):
        refused(hist, lat, targets=targets)
    assert torch.isfinite(pol.attention_saliency_trace(hist, lat, targets=(t for t in [0, 2]))["input_grad"]).all()      # any iterable, read once
    refused(hist, lat, target=torch.zeros(E, S, nA, N))
    refused(hist, lat, targets=[1], target=torch.zeros(E, S, nA, N, A))        # T = 1 targets, a cotangent for S
    refused(hist, lat, target="latent")
    refused(hist, lat, target=A)
    refused(hist, lat, target=1.5)
    refused(hist, lat, gate="soft")
    refused(hist, lat, want=("pair", "maps"))
    refused(hist, lat, noise=torch.zeros(nA, E, S, N, N - 1, 2))              # with deterministic=True
    refused(hist, lat, noise=torch.zeros(nA, E, S, N, N, 2), deterministic=False)
    refused(hist, lat, tau=0.0)
    for pc in (d, 0.0, True, "0"):
        refused(hist, lat, presence_col=pc)
    assert " MB)" in refused(hist, lat, lags=2, max_workspace_mb=0.001)
    assert torch.isfinite(pol.attention_saliency_trace(hist, lat, lags=2)["input_grad"]).all()
    return {}
