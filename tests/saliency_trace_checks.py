"""TEST INFRASTRUCTURE: policy saliency through time (csrc/policy_saliency_lag.hip, ops.saliency_lag, DcntrlMAC.saliency_trace) on whatever
library is active -- the host emulator in tests/test_emu_saliency_trace.py, the gfx950 build in tests/test_gpu_saliency_trace.py.

Ground truth: fp64 torch.autograd.grad through the UNROLLED oracle chain -- oracle.actor_logits / critic_value run step by step on the rows
of saliency_checks.build_rows, the returned hn fed to the next step -- of y_s with respect to every x_j and every entering state; ReLU
trunks take the branch the kernel took (act1 > 0 / act2 > 0 of each row) as ``relu_hint``.  Rule (as
saliency_checks.assert_vs_fp64 applies it), per net, per agent and PER LAG: error = max|got - ref64| / max|ref64| over that lag's valid
rows, bound = max(1e-5, E32_FACTOR x the same chain in fp32 against fp64), for input_grad, gxi, gl1, the carry and the derived
carry_l2 / lag_l1; y (logp, values) at 1e-5.  So that no lag passes vacuously, at every checked lag the fp64 reference's max|g| must be
at least 1e-3 of lag 0's (asserted).  The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors."""
import copy
import inspect
import os

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import _grad_err, _rel
from tests.policy_trace_checks import _bits, _codes, _params, _sync, _worse, assert_out_refused
from tests.saliency_checks import M, TOL, _bound, _learner, _sentinels, _state_tensors, build_rows, entity_sums, get_case

MIN_LAG_RATIO = 1e-3
# (nA, E, S, N, d) + options; lags = S - 1 unless stated.  Slots = E x S: 1, 2 (one link), 15 / 16 / 17 / 65 (tile edges, a second
# workgroup); N = 55 / 64: F at the shipped size and at the limit; d = 4: the contiguous column path; S = 8: a long chain; lags = 2 < S - 1:
# truncated; steps = (1, 4): the chain starts at the slice's start
KERNEL_CASES = [
    ((1, 1, 1, 1, 5), {}),
    ((1, 1, 2, 3, 5), {}),
    ((1, 5, 3, 3, 5), {}),
    ((1, 8, 2, 7, 5), {}),
    ((1, 17, 1, 3, 4), {}),
    ((1, 13, 5, 3, 5), {}),
    ((1, 2, 3, 55, 5), {}),
    ((1, 1, 2, 64, 5), {}),
    ((1, 3, 3, 7, 4), {}),
    ((1, 2, 8, 3, 5), {}),
    ((1, 2, 6, 3, 5), dict(lags=2)),
    ((2, 2, 3, 3, 5), dict(tanh=True)),
    ((1, 2, 3, 3, 5), dict(gat=False)),
    ((1, 2, 3, 7, 5), dict(beh=False)),
    ((1, 2, 3, 3, 5), dict(gat=False, beh=False)),
    ((1, 2, 3, 3, 5), dict(last_action=False)),
    ((2, 2, 3, 3, 5), dict(agent_id=False)),
    ((5, 2, 3, 3, 5), {}),
    ((1, 5, 3, 3, 5), dict(which="actor", target="greedy")),
    ((1, 5, 3, 3, 5), dict(which="critic")),
    ((2, 3, 4, 3, 5), dict(steps=(1, 4))),
    ((1, 2, 3, 3, 5), dict(hidden0="zeros")),
]
CASE_IDS = ["one_slot", "one_link", "slots15", "slots16_ragged_ktile", "slots17_d4_lag0", "slots65_lags4", "N55", "N64", "d4", "chain8_lags7",
            "truncated_lags2", "tanh", "no_gat", "no_beh", "history_only", "no_last_action", "no_agent_id", "five_agents", "actor_only_greedy",
            "critic_only", "steps_1_4", "hidden0_zeros"]
RUN_OPTS = ("which", "target", "steps", "lags", "hidden0")
LAGGED = ("gxi", "gl1", "input_grad", "carry", "carry_l2")                   # keys with the lag axis at dim 2 (lag_l1, lag_valid: dim 1)
ALL_WANT = ("entity", "input_grad", "act", "carry")


def run(case, lags=None, which="both", target="recorded", steps=None, want=ALL_WANT, hidden0=None, batch=None):
    S = case.dims[2]
    steps = slice(0, S) if steps is None else steps
    Sn = steps.stop - steps.start
    res = case.mac.saliency_trace(case.batch if batch is None else batch, Sn - 1 if lags is None else lags, target=target, which=which,
                                  hidden0=hidden0, steps=steps, want=want)
    _sync(case.device)
    return res


def _hidden0(case, i, sl, hidden0):
    """(actor, critic) [E, M] start states of agent i as saliency_trace reads ``hidden0``"""
    f = case.f
    if isinstance(hidden0, str):
        z = torch.zeros(f["history"].shape[0], M)
        return z, z
    if hidden0 is None:
        return f["rnn_states_actors"][:, sl.start, i], f["rnn_states_critics"][:, sl.start, i]
    return torch.as_tensor(hidden0[0])[:, i].cpu(), torch.as_tensor(hidden0[1])[:, i].cpu()


def chain_reference(case, i, dtype, sl, target, hints, hidden0, nets):
    """agent i's nets unrolled over the steps ``sl`` in ``dtype`` -> {net: (y [E,S], G [E,S,S,F], D [E,S,S,M])} and x [E,S,F]:
    G[e, s, j] = d y_s / d x_j and D[e, s, j] = d y_s / d (the state entering step j), total derivatives through the chain (0 for j > s).
    target [E,S] int64; hints: {net: (act1 > 0, act2 > 0) [E,S,M]} or None"""
    f, a = case.f, case.args
    ap, cp = _params(case.mac, dtype)
    x = build_rows(case, i, dtype, sl).clone().requires_grad_(True)
    E, S, F = x.shape
    av = f["avail_actions"][:, sl, i]
    h0 = _hidden0(case, i, sl, hidden0)
    out = {}
    for k, net in enumerate(("actor", "critic")):
        if net not in nets:
            continue
        h = h0[k].to(dtype).clone().requires_grad_(True)
        hin, ys = [], []
        for s in range(S):
            hin.append(h)
            hint = None if hints is None else (hints[net][0][:, s], hints[net][1][:, s])
            if net == "actor":
                logits, h = O.actor_logits(ap[i], x[:, s], h, av[:, s], relu_hint=hint, use_relu=a.use_ReLU)
                ys.append(torch.log_softmax(logits, -1).gather(-1, target[:, s, None])[:, 0])
            else:
                v, h = O.critic_value(cp[i], x[:, s], h, relu_hint=hint, use_relu=a.use_ReLU)
                ys.append(v[:, 0])
        G, D = torch.zeros(E, S, S, F, dtype=dtype), torch.zeros(E, S, S, M, dtype=dtype)
        for s in range(S):
            grads = torch.autograd.grad(ys[s].sum(), [x] + hin[:s + 1], retain_graph=True)
            G[:, s] = grads[0]
            for j in range(s + 1):
                D[:, s, j] = grads[1 + j]
        out[net] = (torch.stack(ys, 1).detach(), G, D)
    return out, x.detach()


def _lag_rows(t, k):
    """[E, S, S, ..] indexed (output step, input step) -> the valid rows of lag k, [E, S - k, ..]: (s, s - k) for s >= k"""
    s = torch.arange(k, t.shape[1])
    return t[:, s, s - k]


def filled_weight(case, sl, batch=None):
    fl = (case.f if batch is None else batch)["filled"]
    return torch.as_tensor(fl).reshape(fl.shape[0], -1)[:, sl].double().cpu()       # [E, S]


def assert_vs_fp64(case, got, sl, K, worst, what, nets=("actor", "critic"), hidden0=None, filled=None):
    """input_grad, gxi, gl1, carry, carry_l2 and lag_l1 of every agent, net and lag against the fp64 chain under the rule; y at 1e-5; the
    vacuity condition on the reference"""
    a = case.args
    S = sl.stop - sl.start
    wt = filled_weight(case, sl) if filled is None else filled
    for i in range(a.n_agents):
        tgt = got["target_action"][:, :, i].cpu() if "target_action" in got else case.f["actions"][:, sl, i, 0]
        hints = None
        if a.use_ReLU:
            hints = {n: (got[n + "_act1"][:, :, i].cpu() > 0, got[n + "_act2"][:, :, i].cpu() > 0) for n in nets}
        r64, x64 = chain_reference(case, i, torch.float64, sl, tgt, hints, hidden0, nets)
        r32, x32 = chain_reference(case, i, torch.float32, sl, tgt, hints, hidden0, nets)
        for net in nets:
            y64, G64, D64 = r64[net]
            _, G32, D32 = r32[net]
            ykey = "logp" if net == "actor" else "values"
            ey = _rel(got[ykey][:, :, i].cpu().flatten(), y64.flatten())
            print(what, net, i, ykey, "err", ey)
            _worse(worst, ykey, ey)
            assert ey <= TOL, (what, net, i, ykey, ey)
            g0 = _lag_rows(G64, 0).abs().max().item()
            for k in range(K + 1):
                g64, g32 = _lag_rows(G64, k).flatten(0, 1), _lag_rows(G32, k).flatten(0, 1)          # [E (S-k), F]
                ratio = g64.abs().max().item() / g0
                _worse(worst, f"{net}_lag{k}_one_over_ratio", 1.0 / max(ratio, 1e-300))
                assert ratio >= MIN_LAG_RATIO, (what, net, i, k, "the reference at this lag is too small to check anything", ratio)
                s_in = torch.arange(k, S) - k
                e64 = entity_sums(case, g64, x64[:, s_in].flatten(0, 1))
                e32 = entity_sums(case, g32, x32[:, s_in].flatten(0, 1))
                d64, d32 = _lag_rows(D64, k), _lag_rows(D32, k)                                      # [E, S-k, M]
                lag = lambda key: got[net + "_" + key][:, k:, k, i].cpu()                            # noqa: E731
                refs = dict(input_grad=(lag("input_grad").flatten(0, 1), g64, g32),
                            gxi=(lag("gxi").flatten(0, 1), e64[0], e32[0]), gl1=(lag("gl1").flatten(0, 1), e64[1], e32[1]),
                            carry=(lag("carry"), d64, d32), carry_l2=(lag("carry_l2"), d64.norm(dim=-1), d32.norm(dim=-1)))
                w = wt[:, k:]                                                                        # [E, S-k]
                if w.sum() > 0:
                    mean = lambda e: ((e.double().sum((-1, -2)).reshape(w.shape) * w).sum() / w.sum()).reshape(1)   # noqa: E731
                    refs["lag_l1"] = (got[net + "_lag_l1"][i, k].cpu().reshape(1), mean(e64[1]), mean(e32[1]))
                else:
                    assert got[net + "_lag_l1"][i, k].item() == 0.0, (what, net, i, k, "lag_l1 without any weight is 0")
                for key, (gv, ref, ref32) in refs.items():
                    assert gv.shape == ref.shape, (key, gv.shape, ref.shape)
                    assert ref.abs().max() > 0, (what, net, key, k, "the reference is zero: the case checks nothing")
                    err, e32_ = _grad_err(gv, ref), _grad_err(ref32, ref)
                    print(what, net, i, "lag", k, key, "err", err, "e32", e32_)
                    _worse(worst, f"{net}_{key}_lag{k}", err)
                    _worse(worst, f"{net}_{key}_lag{k}_e32", e32_)
                    assert err <= _bound(e32_), (what, net, i, k, key, err, e32_)


def assert_invalid_zero(got, K, S):
    """entries with s < k are exactly 0 and lag_valid says which they are"""
    lv = torch.as_tensor(got["lag_valid"]).cpu()
    assert lv.dtype == torch.bool and lv.shape == (S, K + 1)
    assert torch.equal(lv, torch.arange(S)[:, None] >= torch.arange(K + 1)[None, :])
    for key, v in got.items():
        if key.split("_", 1)[-1] in LAGGED:
            v = torch.as_tensor(v).cpu()
            for k in range(1, K + 1):
                assert (v[:, :k, k] == 0).all(), (key, k, "an entry with s < k is not 0")


# ------------------------------------------------------------------------------------------------ the kernel against fp64
def check_kernel(device, dims, opt):
    """1: every lag of input_grad, the entity sums, the carry and the derived quantities of every net and agent against the fp64 chain"""
    runo = {k: v for k, v in opt.items() if k in RUN_OPTS}
    case = get_case(dims, device, tuple(sorted((k, v) for k, v in opt.items() if k not in RUN_OPTS)))
    nA, E, S, N, d = dims
    which = runo.get("which", "both")
    steps = slice(*runo["steps"]) if "steps" in runo else slice(0, S)
    Sn = steps.stop - steps.start
    K = runo.get("lags", Sn - 1)
    hidden0 = runo.get("hidden0")
    got = run(case, lags=K, which=which, target=runo.get("target", "recorded"), steps=steps, hidden0=hidden0)
    nets = ("actor", "critic") if which == "both" else (which,)
    n_src = len(case.mac._widths())
    assert got["sources"] == tuple(k for k, _ in case.mac._widths())
    F = case.mac.input_shape
    shapes = dict(gxi=(E, Sn, K + 1, nA, N, n_src), gl1=(E, Sn, K + 1, nA, N, n_src), input_grad=(E, Sn, K + 1, nA, F), carry=(E, Sn, K + 1, nA, M),
                  carry_l2=(E, Sn, K + 1, nA), act1=(E, Sn, nA, M), act2=(E, Sn, nA, M))
    for net in ("actor", "critic"):
        for key, shape in shapes.items():
            assert (net + "_" + key in got) == (net in nets), (net, key)
            if net in nets:
                assert got[net + "_" + key].shape == shape and got[net + "_" + key].dtype == torch.float32, (net, key, got[net + "_" + key].shape)
        assert ("h_" + net in got) == (net + "_lag_l1" in got) == (net in nets)
        if net in nets:
            assert got["h_" + net].shape == (E, Sn, nA, M)
            assert got[net + "_lag_l1"].shape == (nA, K + 1) and got[net + "_lag_l1"].dtype == torch.float64
    assert ("values" in got) == ("critic" in nets) and ("logp" in got) == ("target_action" in got) == ("actor" in nets)
    if "actor" in nets and runo.get("target", "recorded") == "recorded":
        assert torch.equal(got["target_action"].cpu(), case.f["actions"][:, steps, :, 0])
    assert_invalid_zero(got, K, Sn)
    worst = {}
    assert_vs_fp64(case, got, steps, K, worst, (dims, opt), nets, hidden0)
    return worst


def _same(a, b, what, skip=()):
    keys = sorted(set(a) & set(b))
    assert keys
    for k in keys:
        if k != "sources" and k not in skip:
            x, y = torch.as_tensor(a[k]), torch.as_tensor(b[k])
            assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), (what, k, "bits differ")


def check_lag0(device, dims=(2, 3, 3, 3, 5)):
    """2: lag 0 of every output is saliency(hidden = the entering states) bit for bit; the traced states are policy_trace's bit for bit;
    logp / values agree with policy_trace within 1e-5 and the greedy target is its greedy"""
    case = get_case(dims, device)
    nA, E, S = dims[:3]
    worst = {}
    for target in ("recorded", "greedy"):
        got = run(case, target=target)
        tr = case.mac.policy_trace(case.batch, return_hidden=True)           # walks all S + 1 physical steps; the first S are the window
        _sync(device)
        for net in ("actor", "critic"):
            assert torch.equal(_bits(got["h_" + net]), _bits(tr["h_" + net][:, :S])), (net, "the traced states differ from policy_trace's")
        h0 = (case.batch["rnn_states_actors"][:, 0], case.batch["rnn_states_critics"][:, 0])
        enter = tuple(torch.cat([h.unsqueeze(1), got["h_" + net][:, :-1]], 1) for h, net in zip(h0, ("actor", "critic")))
        sal = case.run(target=target, hidden=enter)
        for key, v in sal.items():
            if key == "sources":
                continue
            mine = got[key][:, :, 0] if key.split("_", 1)[-1] in LAGGED else got[key]
            assert torch.equal(_bits(mine), _bits(v)), (target, key, "lag 0 differs from saliency() on the entering states")
        if target == "greedy":
            assert torch.equal(got["target_action"], tr["greedy"][:, :S]), "greedy target != policy_trace's greedy"
        else:
            for key in ("logp", "values"):
                diff = (got[key] - tr[key][:, :S]).abs().max().item()
                print("saliency_trace vs policy_trace", key, "diff", diff)
                _worse(worst, key + "_vs_trace", diff)
                assert diff <= TOL, (key, diff)
    return worst


def check_prefix(device, dims=(2, 2, 5, 3, 5)):
    """3: the first K' + 1 lags of lags = K equal lags = K' bit for bit"""
    case = get_case(dims, device)
    S = dims[2]
    full = run(case, lags=S - 1)
    for Kp in (0, 1, S - 2):
        part = run(case, lags=Kp)
        cut = {}
        for k, v in full.items():
            if k == "sources":
                continue
            cut[k] = v[:, :, :Kp + 1] if k.split("_", 1)[-1] in LAGGED else (v[:, :Kp + 1] if k.endswith("_lag_l1") or k == "lag_valid" else v)
        _same(part, cut, ("prefix", Kp))
    return {}


def check_placement(device, reps=2):
    """4: repeated calls give the same bits; an environment alone gives the bits it has inside a 17-environment batch; packed and in-place
    fc1 operands give the same bits; a numpy-backed batch gives the bits of the device-backed one"""
    from iplan_amd import synth
    dims = (1, 17, 3, 3, 5)
    case = get_case(dims, device)
    full = run(case)
    for _ in range(reps - 1):
        _same(run(case), full, "repeat")
    per_env = ("actor_lag_l1", "critic_lag_l1", "lag_valid")                 # not per environment: sums over the batch
    for e in (0, 16):
        one = synth.DictBatch({k: v[e:e + 1].clone() for k, v in case.f.items()}, 1, case.T1).to(device)
        alone = run(case, batch=one)
        _same(alone, {k: (v if k == "sources" else v[e:e + 1]) for k, v in full.items() if k not in per_env}, ("alone", e), skip=per_env)
    as_np = run(case, batch=case.np_batch)
    for k, v in full.items():
        if k == "sources":
            assert as_np[k] == v
            continue
        assert isinstance(as_np[k], np.ndarray) and torch.is_tensor(v) and v.device.type == torch.device(device).type, k
        assert np.array_equal(as_np[k], v.cpu().numpy()), (k, "numpy-backed and device-backed batches differ")
    keep = os.environ.get("IPLAN_NO_FC1_PACK")
    os.environ["IPLAN_NO_FC1_PACK"] = "1"                                    # Fc1Pack.get returns None: the arena is read in place
    try:
        assert case.mac.fc1_pack.get(None) is None
        inplace = run(case)
    finally:
        if keep is None:
            del os.environ["IPLAN_NO_FC1_PACK"]
        else:
            os.environ["IPLAN_NO_FC1_PACK"] = keep
    _same(inplace, full, "packed != in place")
    return {}


class _Injected:
    """ops.saliency_lag_args seen through the method: ``out`` is handed to the launches, the descriptors are recorded"""

    def __init__(self, out=None):
        self.out, self.seen = out, None

    def __enter__(self):
        self.orig = ops.saliency_lag_args
        sig = inspect.signature(self.orig)
        inj = self

        def wrapped(*a, **kw):
            b = sig.bind(*a, **kw)
            if inj.out is not None:
                b.arguments["out"] = inj.out
            inj.seen = inj.orig(*b.args, **b.kwargs)
            return inj.seen
        ops.saliency_lag_args = wrapped
        return self

    def __exit__(self, *exc):
        ops.saliency_lag_args = self.orig


OUT_KEYS = ("logp", "values", "target_action", "entity_actor", "entity_critic", "input_grad_actor", "input_grad_critic", "carry_actor", "carry_critic",
            "act1_actor", "act2_actor", "act1_critic", "act2_critic")


def _out_shapes(case, Sn, K):
    nA, E, S, N, d = case.dims
    F, n_src = case.mac.input_shape, len(case.mac._widths())
    sh = dict(logp=(nA, E, Sn), values=(nA, E, Sn), target_action=(nA, E, Sn))
    for net in ("actor", "critic"):
        sh["entity_" + net] = (nA, E, Sn, K + 1, N, n_src, 2)
        sh["input_grad_" + net] = (nA, E, Sn, K + 1, F)
        sh["carry_" + net] = (nA, E, Sn, K + 1, M)
        sh["act1_" + net] = sh["act2_" + net] = (nA, E, Sn, M)
    return sh


def _owned_mask(shape, K):
    """which elements of a lagged output [nA, E, S, K+1, ...] the launches own: s >= k"""
    S = shape[2]
    m = (torch.arange(S)[:, None] >= torch.arange(K + 1)[None, :]).reshape((1, 1, S, K + 1) + (1,) * (len(shape) - 4))
    return m.expand(shape)


def check_sentinel(device):
    """5: at the ops level, outputs carved out of sentinel-filled buffers: nothing outside the owned region is written -- the padding, the
    entries with s < k, an output that was not asked for -- and every owned element is; parameter, gradient and batch bytes unchanged"""
    for dims, opt in (((2, 3, 3, 3, 5), {}), ((1, 17, 2, 7, 5), {}), ((1, 5, 3, 3, 4), dict(gat=False))):
        case = get_case(dims, device, tuple(sorted(opt.items())))
        S = dims[2]
        K = S - 1
        shapes = _out_shapes(case, S, K)
        watched = [case.mac.actor_arena.data, case.mac.critic_arena.data, case.mac.actor_arena.grad, case.mac.critic_arena.grad] + \
            [v for v in case.batch.data.values() if torch.is_tensor(v)]
        before = [t.clone() for t in watched]
        with _Injected() as inj:
            run(case)
            ref = dict(inj.seen[1])
        assert set(ref) == set(OUT_KEYS), sorted(ref)
        for which, want in (("both", ALL_WANT), ("both", ("entity",)), ("actor", ("input_grad",)), ("critic", ())):
            bufs = _sentinels(shapes, device)
            with _Injected(out={k: v[2] for k, v in bufs.items()}) as inj:
                run(case, which=which, want=want)
                got = dict(inj.seen[1])
            nets = ("actor", "critic") if which == "both" else (which,)
            asked = ("entity",) + tuple(w for w in want if w in ("input_grad", "act"))           # the method always takes the entity sums
            owned = {k for k in OUT_KEYS if (k in ("logp", "target_action") and "actor" in nets) or (k == "values" and "critic" in nets)
                     or any(k == "carry_" + n for n in nets)
                     or any(k == w + "_" + n or (w == "act" and k in ("act1_" + n, "act2_" + n)) for w in asked for n in nets)}
            assert set(got) == owned, (which, want, sorted(got), sorted(owned))
            for k, (sent, buf, view) in bufs.items():
                host = buf.cpu()
                if k not in owned:
                    assert torch.equal(host, sent), (dims, which, want, k, "was not asked for and was written")
                    continue
                n = view.numel()
                assert torch.equal(host[:32], sent[:32]) and torch.equal(host[32 + n:], sent[32 + n:]), (dims, k, "an element outside the owned region was written")
                inner, sin = host[32:32 + n].view(view.shape), sent[32:32 + n].view(view.shape)
                if len(view.shape) > 4 or k.startswith("carry"):
                    own = _owned_mask(view.shape, K)
                    assert torch.equal(_bits(inner[~own]), _bits(sin[~own])), (dims, k, "an entry with s < k was written")
                    assert torch.equal(_bits(inner[own]), _bits(ref[k].cpu()[own])), (dims, k, "differs inside a padded buffer")
                else:
                    assert torch.equal(_bits(inner), _bits(ref[k].cpu())), (dims, k, "differs inside a padded buffer")
        b2 = _sentinels(shapes, device, 0.25)                 # every owned element is written: a second, shifted sentinel ends the same
        with _Injected(out={k: v[2] for k, v in b2.items()}):
            run(case)
        for k in OUT_KEYS:
            v, r = b2[k][2].cpu(), ref[k].cpu()
            own = _owned_mask(v.shape, K) if (len(v.shape) > 4 or k.startswith("carry")) else torch.ones(v.shape, dtype=torch.bool)
            assert torch.equal(_bits(v[own]), _bits(r[own])), (dims, k, "an owned element was left unwritten")
        _sync(device)
        for t, b in zip(watched, before):
            assert torch.equal(t, b), (dims, "parameter, gradient or batch bytes changed", tuple(t.shape))
    return {}


def check_touches_nothing(device):
    """6: parameters, both arenas' gradient entries (pre-filled with a sentinel), the optimisers' state, hidden_states, the batch and
    the torch generator states are bit-identical before and after saliency_trace(); a train() after it gives the bits of one without
    it (saliency_checks.check_touches_nothing, for this method)"""
    results = []
    for with_call in (False, True):
        args, mac, learner, batch = _learner(device)
        torch.manual_seed(83)
        if with_call:
            for arena in (mac.actor_arena, mac.critic_arena):
                arena.grad.fill_(0.7071)
            watched = [t for t in _state_tensors(learner) if t.device.type == torch.device(device).type]
            assert any(t.data_ptr() == mac.actor_arena.data.data_ptr() for t in watched) and len(watched) > 8, len(watched)
            before = [t.clone() for t in watched]
            fields = {k: v.clone() for k, v in batch.data.items()}
            states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None)
            mac.hidden_states = "untouched"
            res = mac.saliency_trace(batch, 3, want=("entity", "input_grad"))
            _sync(device)
            assert torch.isfinite(res["actor_gxi"]).all() and torch.isfinite(res["critic_input_grad"]).all()
            assert (res["actor_gl1"][:, 3:, 3].abs().sum() > 0) and (res["critic_carry_l2"][:, 3:, 3] > 0).all()
            assert torch.equal(torch.get_rng_state(), states[0])
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


def check_filled_weighting(device, dims=(2, 3, 4, 3, 5)):
    """7: lag_l1 weighs the rows with batch["filled"]: a batch whose later steps are unfilled -- environment 0 from step 2 on, every
    environment at the last step -- against the fp64 chain under the rule; the lag whose rows are all unfilled gives exactly 0; the
    gradients themselves do not depend on ``filled``"""
    from iplan_amd import synth
    case = get_case(dims, device)
    nA, E, S = dims[:3]
    f = {k: v.clone() for k, v in case.f.items()}
    f["filled"][0, 2:] = 0
    f["filled"][:, S - 1:] = 0
    f["filled"][1:, :S - 1] = 1
    batch = synth.DictBatch(f, E, case.T1).to(device)
    got = run(case, batch=batch)
    plain = run(case)
    _same(got, plain, "filled changes more than lag_l1", skip=("actor_lag_l1", "critic_lag_l1"))
    worst = {}
    assert_vs_fp64(case, got, slice(0, S), S - 1, worst, "unfilled later steps", filled=filled_weight(case, slice(0, S), f))
    for net in ("actor", "critic"):
        assert (got[net + "_lag_l1"][:, S - 1] == 0).all() and (got[net + "_lag_l1"][:, :S - 1] > 0).all()
        assert not torch.equal(got[net + "_lag_l1"], plain[net + "_lag_l1"])
        # the same numbers from the method's own per-row outputs, in float64
        row = got[net + "_gl1"].double().sum((-1, -2)).cpu()                                      # [E, S, K+1, nA]
        wt = filled_weight(case, slice(0, S), f)
        for k in range(S - 1):
            ref = (row[:, k:, k] * wt[:, k:, None]).sum((0, 1)) / wt[:, k:].sum()
            assert torch.allclose(got[net + "_lag_l1"][:, k].cpu(), ref, rtol=1e-12, atol=0), (net, k)
    return worst


def check_bad_arguments(device, dims=(2, 3, 3, 3, 5)):
    """8: lags outside [0, S - 1] or not an int, and a slice with a step other than 1, raise ValueError; layer_N = 2 raises
    NotImplementedError; an ``out=`` destination of the wrong shape or dtype, or a non-contiguous one, makes ops.saliency_lag raise
    AssertionError; at the C level each check of iplan_ac_saliency_lag returns its error code with a message and nothing is launched,
    so the sentinel-filled outputs stay as they were"""
    case = get_case(dims, device)
    S = dims[2]
    K = S - 1
    good = run(case)
    for bad in (dict(lags=-1), dict(lags=S), dict(lags=1.0), dict(lags=0, steps=slice(0, S, 2)), dict(lags=2, steps=slice(1, S))):
        try:
            case.mac.saliency_trace(case.batch, bad["lags"], steps=bad.get("steps", slice(0, S)))
        except ValueError:
            pass
        else:
            raise AssertionError(f"{bad} was not refused")
    bufs = _sentinels(_out_shapes(case, S, K), device)
    with _Injected(out={k: v[2] for k, v in bufs.items()}) as inj:
        run(case)
        launches, res, keep = inj.seen
    fresh = _sentinels(_out_shapes(case, S, K), device)
    for k, v in fresh.items():                                               # back to sentinels: only the refused calls follow
        bufs[k][1].copy_(v[1])
    _sync(device)
    lib = ops._lib(None)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iplan_hip.h")).read()
    import re
    EALIGN = int(re.search(r"IPLAN_EALIGN\s*=\s*(-?\d+)", text).group(1))
    EINVAL = _codes()
    fn = lib.c.iplan_ac_saliency_lag

    def refused(x, code=EINVAL, **fields):
        keep_f = {}
        for k, v in fields.items():
            obj, name = (x, k) if "." not in k else (getattr(x, k.split(".")[0]), k.split(".")[1])
            keep_f[k] = (obj, name, getattr(obj, name))
            setattr(obj, name, v)
        rc = fn(L.C.byref(x) if x is not None else None, L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for obj, name, v in keep_f.values():
            setattr(obj, name, v)
        assert rc == code and rc < 0 and "iplan_ac_saliency" in msg, (fields, rc, msg)
        return msg

    x0, x1, xl = launches[0], launches[1], launches[K]
    assert "iplan_ac_saliency_lag" in refused(None)
    for x in (x0, x1):
        assert "iplan_ac_saliency_lag" in refused(x, lag=-1)
        assert "iplan_ac_saliency_lag" in refused(x, lag=K + 1)              # lag >= n_lags
        assert "iplan_ac_saliency_lag" in refused(x, n_lags=0)
        assert "iplan_ac_saliency_lag" in refused(x, n_lags=S + 1)           # lags reach before the first step
        refused(x, **{"base.S": 0})                                          # the row description: iplan_ac_saliency's checks
        refused(x, **{"base.which": 3})
        refused(x, **{"base.h_actor": None})
    assert "seed" in refused(x1, seed_actor=None)
    assert "seed" in refused(x1, seed_critic=None)
    assert "seed" in refused(xl, seed_actor=None)
    assert "carry" in refused(x0, carry_actor=None)
    assert "carry" in refused(x1, carry_critic=None)
    assert "seed_s_row" in refused(x1, seed_s_row=32)
    assert "carry_s_row" in refused(x0, carry_s_row=0)
    refused(x0, carry_s_row=-64)
    none = {"base." + k: None for k in ("logp", "values", "target_out", "entity_actor", "entity_critic", "input_grad_actor", "input_grad_critic",
                                         "act1_actor", "act2_actor", "act1_critic", "act2_critic")}
    assert "no output" in refused(xl, carry_actor=None, carry_critic=None, **none)
    # lag >= 1 writes no y and no act: with only those asked for there is nothing to write
    assert "no output" in refused(xl, carry_actor=None, carry_critic=None, **{k: None for k in none if "entity" in k or "input_grad" in k})
    refused(x1, code=EALIGN, seed_actor=x1.seed_actor + 4)
    refused(x0, code=EALIGN, carry_critic=x0.carry_critic + 8)
    refused(x0, code=EALIGN, carry_s_row=M + 2)
    refused(x1, code=EALIGN, seed_s_row=M + 1)
    refused(x0, code=EALIGN, **{"base.act1_actor": x0.base.act1_actor + 4})

    def with_out(out):                                                       # ops.saliency_lag, called by the method with this ``out``
        with _Injected(out=out):
            run(case)
    assert_out_refused(with_out, bufs, ("carry_actor", "entity_critic", "target_action"))
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(buf.cpu(), sent), (k, "a refused call wrote an output")
    _same(run(case), good, "after the refusals")
    del keep, res
    mac = case.mac
    orig = mac.args
    try:
        mac.args = copy.copy(orig)
        mac.args.layer_N = 2
        try:
            mac.saliency_trace(case.batch, 1)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("layer_N = 2 was not refused")
        mac.args.layer_N, mac.args.recurrent_N = 1, 2
        try:
            mac.saliency_trace(case.batch, 1)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("recurrent_N = 2 was not refused")
    finally:
        mac.args = orig
    return {}
