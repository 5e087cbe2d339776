"""TEST INFRASTRUCTURE: the actor / critic backward alone (csrc/actor_critic_bwd.hip, csrc/ac_fc1_split.hip and the 64-wide wgrad jobs
through ops.ac_backward: iplan_ac_bwd_tail, iplan_ac_bwd_fc1 or iplan_ac_bwd_fc1_split, iplan_wgrad, iplan_ac_bwd_fc1_finalize) on
whatever library is active -- the host emulator in tests/test_emu_ac_backward.py, the gfx950 build in tests/test_gpu_ac_backward.py.

Case: ac_forward_checks.AcCase (spread parameters, LayerNorm affines included; strided views with T_phys = S + 1; a GRU state per row;
a row with one available action and a last row with none; junk around the recorded actions).  The forward is ``case.run(form, mp,
which=..., save=True)``; the backward forms are the fp32 contraction after a ``stream`` / ``stats`` / ``module`` forward and the
split-bf16 contraction after a ``pre`` forward.

Ground truth: fp64 autograd of oracle.actor_evaluate + oracle.actor_logits (per-row entropies) and oracle.critic_value on
``case.features(i, float64)``, every row with its own recorded state; losses sum(logp g_logp) + sum(g_entropy entropy_row) and
sum(values g_values); the same in fp32 beside it.  Row-level gradients are those of a zero [rows, width] tensor added to the layer's
bias (the oracle's own code, unchanged: the gradient of a pre-activation is the gradient of what is added to it).  ReLU trunks take
the branch the launch took (saved slots a1 / a2 > 0) as ``relu_hint`` at units within 1e-5 of the kink; the hinted units that differ
from fp64's own branch are counted per net from oracle.RELU_HINT_LOG and capped at oracle_checks.RELU_HINT_MAX.
Rule (tests/oracle_checks.py, policy_trace_checks._bound): error = max|got - ref64| / max|ref64| per tensor and net, bound =
max(1e-5, E32_FACTOR x e32).  A tensor whose fp64 gradient is identically zero (one action: logp = 0) must be exactly zero.
The checks never touch ``L.use_library_for_tests``; each returns what it measured."""
import ctypes as C
import hashlib
import types

import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import ac_forward_checks as AC
from tests import policy_trace_checks as PC
from tests.oracle_checks import RELU_HINT_MAX, _grad_err
from tests.policy_trace_checks import M, _bits, _bound, _sync, _worse

FORMS = ("stream", "stats", "module", "pre")
FP32_FORMS = ("stream", "stats", "module")
# rows -> (E, S): a single row; one full tile; T = 1; T = 16 (adv_t == 0); a third tile at T = 3; T > 16 (adv_ep == 0); the edges of the
# tail's 128-row workgroup; a second fp32 chunk of one row, and of two rows starting at step 1 of episode 85
ROWS = {1: (1, 1), 16: (8, 2), 17: (17, 1), 32: (2, 16), 33: (11, 3), 34: (2, 17), 127: (127, 1), 128: (32, 4), 129: (43, 3), 257: (257, 1),
        258: (86, 3)}


def dims_of(rows, nA=2, N=3, d=5, n_act=5):
    E, S = ROWS[rows]
    return (nA, E, S, N, d, n_act)


# K axis, 17 rows: the forward suite's cases as they stand, the int64 last action read in place, and N = 12 -- an attention block of 24
# k-tiles (three fc1 groups of 8) in 35 k-tiles (a second 32-tile k-block of the split kernel with three live tiles)
K_CASES = list(AC.K_CASES) + [("last64", dims_of(17), dict(last64=True)), ("N12", dims_of(17, N=12), {})]
CASES = {f"rows{r}": (dims_of(r), {}) for r in ROWS}
CASES.update({"k_" + c[0]: (c[1], c[2]) for c in K_CASES})
# seed of every case, chosen on the CPU from the oracle alone (pick_seed): the first at which the fp32 oracle's own ReLU branches,
# handed to the fp64 oracle as the hint, differ from fp64's branches at no more than RELU_HINT_MAX units per net
SEEDS = {name: 0 for name in CASES}
FC1_TENSORS = ("base.mlp.fc1.0.weight", "base.feature_norm.weight", "base.feature_norm.bias")
KINDS = ("actor", "critic")
HEAD_BIAS = ("act.action_out.linear.bias", "v_out.bias")
# parameters fp64 autograd gives no gradient: the template layer that layer_N = 1 never calls, PopArt's running statistics
NO_GRAD = ("base.mlp.fc_h.0.weight", "base.mlp.fc_h.0.bias", "base.mlp.fc_h.2.weight", "base.mlp.fc_h.2.bias", "v_out.stddev", "v_out.mean",
           "v_out.mean_sq", "v_out.debiasing_term")
FENCE = 1024
POISON = 16384          # floats of NaN around the replays' dsave: more than the 31 rows a 32-row step can reach past the end


def case_of(name, device, poison=False):
    dims, opt = CASES[name]
    return AC.get_case(dims, device, AC._opt(opt), seed=SEEDS[name], poison=poison)


def _kinds(which):
    return (0, 1) if which == 2 else (which,)


def _sentinel(n, device):
    return (2.5 + (torch.arange(n, dtype=torch.float32) % 1021) / 1024.0).to(device)


def _group(name):
    if name in FC1_TENSORS:
        return "fc1"
    return "ln" if ("norm" in name or name.startswith(("base.mlp.fc1.2", "base.mlp.fc2.0.2"))) else "wide64"


# ------------------------------------------------------------------------------------------------ upstream gradients and the reference
def upstream(case):
    """g_logp, g_values (randn + 0.5: the row-sum gradients v_out.bias / rnn.norm.bias do not cancel) and the per-row g_entropy
    (0.01 randn), [nA, rows] each, from a fixed generator; computed once per case"""
    if "_bwd_up" not in case.__dict__:
        nA, E, S = case.dims[:3]
        gen = torch.Generator().manual_seed(1700 + E * S)
        case._bwd_up = dict(g_logp=torch.randn(nA, E * S, generator=gen) + 0.5, g_values=torch.randn(nA, E * S, generator=gen) + 0.5,
                            g_entropy=0.01 * torch.randn(nA, E * S, generator=gen))
    return case._bwd_up


def _row_biases(kind):
    return dict(dz1="base.mlp.fc1.0.bias", dz2="base.mlp.fc2.0.0.bias", gi="rnn.rnn.bias_ih_l0", gh="rnn.rnn.bias_hh_l0", dhead=HEAD_BIAS[kind])


def _net_reference(case, kind, i, dtype, hint, ent_rows):
    nA, E, S, N, d, n_act = case.dims
    rows = E * S
    up = upstream(case)
    p = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in PC._params(case.mac, dtype)[kind][i].items()}
    q, delta = dict(p), {}
    for key, name in _row_biases(kind).items():
        delta[key] = torch.zeros(rows, p[name].shape[0], dtype=dtype, requires_grad=True)
        q[name] = p[name] + delta[key]
    f = case.fields(i)
    x = case.features(i, dtype).reshape(rows, -1)
    h = case.buf["hc" if kind else "ha"][:, :S, i, 4:4 + M].reshape(rows, M).to(dtype)
    relu = case.args.use_ReLU
    hint = hint if relu else None
    O.RELU_HINT_LOG.clear()
    if kind == 0:
        av = f["avail"].reshape(rows, n_act)
        lp, _ = O.actor_evaluate(q, x, h, f["actions"].reshape(rows), av, relu_hint=hint, use_relu=relu)
        logits, _ = O.actor_logits(q, x, h, av, relu_hint=hint, use_relu=relu)
        la = torch.log_softmax(logits, -1)
        ent = -(la.exp() * la.clamp_min(torch.finfo(dtype).min)).sum(-1)
        g_ent = up["g_entropy"][i].to(dtype) if ent_rows else torch.full((rows,), -0.01 / rows, dtype=dtype)
        loss = (lp[:, 0] * up["g_logp"][i].to(dtype)).sum() + (g_ent * ent).sum()
    else:
        v, _ = O.critic_value(q, x, h, relu_hint=hint, use_relu=relu)
        loss = (v[:, 0] * up["g_values"][i].to(dtype)).sum()
    log = list(O.RELU_HINT_LOG[:2])                       # (fc1, fc2) of the first trunk evaluation; the actor's second is the same
    loss.backward()
    rowg = {k: v.grad for k, v in delta.items()}
    return types.SimpleNamespace(grads={k: v.grad for k, v in p.items() if v.grad is not None},
                                 rows=rowg,
                                 ambiguous=sum(a for a, _ in log), differ=sum(b for _, b in log))


def reference(case, kind, i, dtype, hint, ent_rows=False):
    """fp64 / fp32 autograd of net (kind, i): cached per case, net, dtype, entropy form and hint bits; never modified"""
    cache = case.__dict__.setdefault("_bwd_ref", {})
    hk = None if hint is None else hashlib.sha1(hint[0].numpy().tobytes() + hint[1].numpy().tobytes()).hexdigest()
    key = (kind, i, dtype, ent_rows, hk)
    if key not in cache:
        cache[key] = _net_reference(case, kind, i, dtype, hint, ent_rows)
    return cache[key]


def _fp32_branches(p, x):
    """the (fc1, fc2) ReLU branches of the fp32 oracle's own forward (oracle.ac_trunk's first two layers)"""
    f = O.layer_norm(x, p["base.feature_norm.weight"], p["base.feature_norm.bias"])
    z1 = f @ p["base.mlp.fc1.0.weight"].t() + p["base.mlp.fc1.0.bias"]
    f = O.layer_norm(torch.relu(z1), p["base.mlp.fc1.2.weight"], p["base.mlp.fc1.2.bias"])
    return z1 > 0, f @ p["base.mlp.fc2.0.0.weight"].t() + p["base.mlp.fc2.0.0.bias"] > 0


def hint_differences(case):
    """the fp32 oracle's own branches handed to the fp64 oracle as hints: the largest count, over the nets, of hinted units that differ"""
    nA, E, S = case.dims[:3]
    rows = E * S
    if not case.args.use_ReLU:
        return 0
    worst = 0
    for kind in (0, 1):
        p32, p64 = PC._params(case.mac, torch.float32)[kind], PC._params(case.mac, torch.float64)[kind]
        for i in range(nA):
            hint = _fp32_branches(p32[i], case.features(i, torch.float32).reshape(rows, -1))
            h = case.buf["hc" if kind else "ha"][:, :S, i, 4:4 + M].reshape(rows, M).double()
            O.RELU_HINT_LOG.clear()
            O.ac_trunk(p64[i], case.features(i, torch.float64).reshape(rows, -1), h, hint)
            worst = max(worst, sum(b for _, b in O.RELU_HINT_LOG))
    return worst


def pick_seed(name, tries=20):
    """the first seed of case ``name`` at which the fp32 oracle's forward alone stays within RELU_HINT_MAX (CPU, oracle only)"""
    dims, opt = CASES[name]
    for seed in range(tries):
        if hint_differences(AC.get_case(dims, "cpu", AC._opt(opt), seed=seed)) <= RELU_HINT_MAX:
            return seed
    raise AssertionError("no seed found")


# ------------------------------------------------------------------------------------------------ running the backward
def _stream(device):
    return C.c_void_p(L.current_stream(torch.device(device)) or 0)


def _copy_args(a):
    return L.AcBwdArgs.from_buffer_copy(a)


def run_backward(case, form, mp, which=2, ent_rows=False, fwd=None, sentinel=True):
    """the forward in ``form`` (or ``fwd``) and ops.ac_backward on it, both arenas sentinel-filled first.  Returns the descriptor the
    library saw (recorded from lib.call: the chunking is what ops.ac_backward chose, not a restatement of it)"""
    device, mac = case.device, case.mac
    lib = ops._lib(None)
    if fwd is None:
        fwd = case.run(form, mp, which=which, save=True)
    up = upstream(case)
    E, S, nA = len(case.order), case.dims[2], case.dims[0]
    perm = lambda t: t.reshape(nA, case.dims[1], S)[:, case.order].reshape(nA, E * S).contiguous().to(device)  # noqa: E731
    dev_up = {k: perm(v) for k, v in up.items()}
    sent = {}
    for kind, arena in enumerate((mac.actor_arena, mac.critic_arena)):
        sent[kind] = _sentinel(arena.grad.numel(), "cpu").view(arena.grad.shape)
        if sentinel:
            arena.grad.copy_(sent[kind])
    calls = []
    real = L.Lib.call.__get__(lib)

    def spy(name, args, stream=None):
        calls.append((name, args))
        return real(name, args, stream)

    lib.call = spy
    try:
        res = ops.ac_backward(fwd, mac.actor_arena, mac.critic_arena, g_logp=dev_up["g_logp"],
                              g_entropy=dev_up["g_entropy"] if ent_rows else -0.01 / (case.dims[1] * S), g_values=dev_up["g_values"])
    finally:
        del lib.call
    _sync(device)
    args = [a for n, a in calls if n == "iplan_ac_bwd_tail"][0]
    saved = fwd["saved"].cpu()
    return types.SimpleNamespace(case=case, form=form, which=which, ent_rows=ent_rows, fwd=fwd, dsave=res["dsave"], ln_part=res["ln_part"],
                                 args=args, entry_points=[n for n, _ in calls], keep=dev_up, sentinel=sent, saved=saved,
                                 grads=[mac.actor_arena.grad.cpu().clone(), mac.critic_arena.grad.cpu().clone()])


def _hint(run, kind, i):
    """(fc1, fc2) branches of the launch itself.  After case.upload(order) the rows are brought back to the case's own order"""
    case = run.case
    nA, E, S = case.dims[:3]
    sv = run.saved[kind, i]
    if len(case.order) == E and not torch.equal(case.order, torch.arange(E)):
        inv = torch.argsort(case.order)
        sv = sv.reshape(E, S, -1)[inv].reshape(E * S, -1)
    return sv[:, 0:M] > 0, sv[:, 2 * M:3 * M] > 0


def compare_grads(run, worst, what, names=None, grads=None):
    """every parameter gradient of the nets that took part against fp64 under the rule -> the names compared, per kind"""
    case = run.case
    nA = case.dims[0]
    arenas = (case.mac.actor_arena, case.mac.critic_arena)
    grads = run.grads if grads is None else grads
    done = {}
    for kind in _kinds(run.which):
        for i in range(nA):
            hint = _hint(run, kind, i)
            r64, r32 = (reference(case, kind, i, dt, hint, run.ent_rows) for dt in (torch.float64, torch.float32))
            _worse(worst, "relu_hint_ambiguous", r64.ambiguous)
            _worse(worst, "relu_hint_differ", r64.differ)
            assert r64.differ <= RELU_HINT_MAX, (what, KINDS[kind], i, "ReLU branches taken from the launch under test", r64.differ)
            done[kind] = sorted(r64.grads)
            for name, g64 in r64.grads.items():
                if names is not None and name not in names:
                    continue
                o, n = arenas[kind].off(name), g64.numel()
                got = grads[kind][i, o:o + n].view(g64.shape)
                assert torch.isfinite(got).all(), (what, KINDS[kind], i, name, "not finite")
                if float(g64.abs().max()) == 0.0:
                    assert not got.any(), (what, KINDS[kind], i, name, "fp64 gradient is identically zero, the kernel's is not")
                    continue
                err, e32 = _grad_err(got, g64), _grad_err(r32.grads[name], g64)
                print(what, KINDS[kind], i, name, "err", err, "e32", e32)
                key = KINDS[kind] + "_" + _group(name)
                _worse(worst, key, err)
                _worse(worst, key + "_e32", e32)
                assert err <= _bound(e32), (what, KINDS[kind], i, name, err, e32)
    return done


# ------------------------------------------------------------------------------------------------ 1, 2: every gradient against fp64
def check_vs_fp64(device, mp, form, name):
    """every actor and critic parameter gradient of every net against fp64 under the rule, after a forward in ``form``; the chunk
    count of the contraction (two fp32 chunks at 257 / 258 rows; what iplan_ac_fc1_split_chunks returns for the split form); N12:
    three attention groups, 35 k-tiles"""
    case = case_of(name, device)
    lib = ops._lib(None)
    rows = case.rows
    run = run_backward(case, form, mp)
    a = run.args
    worst = {}
    if form == "pre":
        cr = C.c_int32(0)
        n = lib.c.iplan_ac_fc1_split_chunks(C.byref(a.fwd.feat), case.dims[0], rows, C.byref(cr))
        assert "iplan_ac_bwd_fc1_split" in run.entry_points and "iplan_ac_bwd_fc1" not in run.entry_points
        assert a.fc1_chunk_rows == cr.value and a.fc1_chunks == n == (rows + cr.value - 1) // cr.value, (a.fc1_chunks, a.fc1_chunk_rows, n, cr.value)
    else:
        assert "iplan_ac_bwd_fc1" in run.entry_points and "iplan_ac_bwd_fc1_split" not in run.entry_points
        assert a.fc1_chunks == (rows + a.fc1_chunk_rows - 1) // a.fc1_chunk_rows
        if rows in (257, 258):
            assert a.fc1_chunks == 2, (rows, a.fc1_chunks, a.fc1_chunk_rows)
    if name == "k_N12":
        groups, kt = int(lib.c.iplan_ac_fc1_groups(C.byref(a.fwd.feat))), int(lib.c.iplan_ac_kpad(C.byref(a.fwd.feat))) // 16
        # history 60 -> 4 k-tiles (1 group), attention 384 -> 24 (3 groups of 8), behaviour 96 -> 6 (1), one-hots 7 -> 1 (1)
        assert groups == 6 and kt == 35, (groups, kt)
    done = compare_grads(run, worst, (form, name))
    assert set(done) == {0, 1} and all(len(v) >= 18 for v in done.values()), done
    return worst


# ------------------------------------------------------------------------------------------------ 3: which and ownership
def _fenced(n, device):
    """n floats inside a sentinel-filled buffer with FENCE floats on either side -> (host sentinel, device buffer, view)"""
    sent = _sentinel(n + 2 * FENCE, "cpu")
    buf = sent.clone().to(device)
    return sent, buf, buf[FENCE:FENCE + n]


def _fence_intact(fenced, what):
    sent, buf, _ = fenced
    host = buf.cpu()
    assert torch.equal(_bits(host[:FENCE]), _bits(sent[:FENCE])) and torch.equal(_bits(host[-FENCE:]), _bits(sent[-FENCE:])), (what, "wrote outside its buffer")


def check_which(device, mp, form, which, rows=33):
    """which = 0 / 1 / 2 on sentinel-filled arenas: every parameter fp64 autograd gives a gradient meets the rule (overwritten, not
    added to); the arena of a net kind that did not take part keeps the sentinel's bits; arena entries of tensors without an fp64
    gradient (NO_GRAD: base.mlp.fc_h.*, PopArt's statistics) and the alignment gaps between tensors KEEP THE
    SENTINEL: the backward writes nothing there, zeroing them is the optimiser's zero_grad.  Then the tail is
    replayed on dsave / ln_part placed inside larger sentinel-filled buffers: the bits of ops.ac_backward's own, nothing outside
    [2, nA, rows, ...] / [2, nA, tiles, ...] changed, and the half of a net kind that did not take part untouched"""
    case = case_of(f"rows{rows}", device)
    lib = ops._lib(None)
    nA = case.dims[0]
    run = run_backward(case, form, mp, which=which)
    worst = {}
    done = compare_grads(run, worst, (form, "which", which))
    assert set(done) == set(_kinds(which))
    for kind, arena in enumerate((case.mac.actor_arena, case.mac.critic_arena)):
        owned = torch.zeros(arena.grad.shape, dtype=torch.bool)
        if kind in done:
            assert set(arena.names) - set(done[kind]) == set(NO_GRAD) & set(arena.names)
            for o, n in arena.ranges(done[kind]):
                owned[:, o:o + n] = True
        got, sent = run.grads[kind], run.sentinel[kind]
        assert torch.equal(_bits(got[~owned]), _bits(sent[~owned])), (form, which, KINDS[kind], "an arena entry outside the launch's tensors was written")
    # the tail again, on fenced row buffers
    tiles = (rows + 15) // 16
    ds, lp = _fenced(2 * nA * rows * L.AC_DSAVE_FLOATS, device), _fenced(2 * nA * tiles * L.AC_LNPART_FLOATS, device)
    a = _copy_args(run.args)
    a.dsave, a.ln_part = ds[2].data_ptr(), lp[2].data_ptr()
    rc = lib.c.iplan_ac_bwd_tail(C.byref(a), _stream(device))
    _sync(device)
    assert rc == 0, lib.c.iplan_last_error().decode()
    _fence_intact(ds, "dsave")
    _fence_intact(lp, "ln_part")
    for (sent, buf, view), own, width in ((ds, run.dsave, rows * L.AC_DSAVE_FLOATS), (lp, run.ln_part, tiles * L.AC_LNPART_FLOATS)):
        view = view.view(2, nA, width)
        for kind in (0, 1):
            if kind in _kinds(which):
                assert torch.equal(_bits(view[kind]), _bits(own.view(2, nA, width)[kind])), (form, which, KINDS[kind], "the replayed tail differs")
            else:
                assert torch.equal(_bits(view[kind].cpu()), _bits(sent[FENCE:-FENCE].view(2, nA, width)[kind])), \
                    (form, which, KINDS[kind], "written without taking part")
    return worst


# ------------------------------------------------------------------------------------------------ 4: row-level gradients, head edges
def check_rows(device, mp, form, rows, ent_rows):
    """dsave's dz1, dz2, the four gate blocks and dhead[:n_out] against fp64 under the rule; dhead exactly zero at every unavailable
    action (the row with no available action included: the gradient of the oracle's torch.where) and in columns >= n_out; everything
    finite although masked actions have probability exactly zero in the entropy term; every parameter gradient under the rule too
    (``ent_rows``: the per-row g_entropy tensor instead of the constant)"""
    case = case_of(f"rows{rows}", device)
    nA, n_act = case.dims[0], case.dims[5]
    run = run_backward(case, form, mp, ent_rows=ent_rows)
    what = (form, rows, "g_entropy rows" if ent_rows else "g_entropy const")
    worst = {}
    compare_grads(run, worst, what)
    ds = run.dsave.cpu()
    assert torch.isfinite(ds).all() and torch.isfinite(run.ln_part).all(), (what, "not finite")
    avail = case.avail_rows()
    none_i, none_r = case.row_index(case.none_row)
    assert int(avail[none_i, none_r].sum()) == 0 and (avail.sum(-1) == 1).any()
    for kind in (0, 1):
        n_out = n_act if kind == 0 else 1
        for i in range(nA):
            hint = _hint(run, kind, i)
            r64, r32 = (reference(case, kind, i, dt, hint, ent_rows) for dt in (torch.float64, torch.float32))
            d = ds[kind, i]
            blocks = dict(dz1=(d[:, 0:M], lambda g: g["dz1"]), dz2=(d[:, M:2 * M], lambda g: g["dz2"]),
                          dr=(d[:, 2 * M:3 * M], lambda g: g["gi"][:, 0:M]), dz=(d[:, 3 * M:4 * M], lambda g: g["gi"][:, M:2 * M]),
                          dni=(d[:, 4 * M:5 * M], lambda g: g["gi"][:, 2 * M:]), dnh=(d[:, 5 * M:6 * M], lambda g: g["gh"][:, 2 * M:]),
                          dhead=(d[:, 6 * M:6 * M + n_out], lambda g: g["dhead"]))
            assert torch.equal(r64.rows["gi"][:, :2 * M], r64.rows["gh"][:, :2 * M])
            for key, (got, pick) in blocks.items():
                g64, g32 = pick(r64.rows), pick(r32.rows)
                assert got.shape == g64.shape and float(g64.abs().max()) > 0, (what, key, got.shape)
                err, e32 = _grad_err(got, g64), _grad_err(g32, g64)
                print(what, KINDS[kind], i, key, "err", err, "e32", e32)
                _worse(worst, "row_" + key, err)
                _worse(worst, "row_" + key + "_e32", e32)
                assert err <= _bound(e32), (what, KINDS[kind], i, key, err, e32)
            assert not d[:, 6 * M + n_out:6 * M + 16].any(), (what, KINDS[kind], i, "dhead is non-zero in a column >= n_out")
            if kind == 0:
                masked = avail[i] == 0
                assert not d[:, 6 * M:6 * M + n_act][masked].any(), (what, i, "dhead is non-zero at an unavailable action")
                assert not r64.rows["dhead"][masked].any()
    return worst


# ------------------------------------------------------------------------------------------------ 5: same bits where promised
def _same(a, b, what):
    for k in (0, 1):
        assert torch.equal(_bits(a.grads[k]), _bits(b.grads[k])), (what, KINDS[k], "gradient arena: bits differ")
    assert torch.equal(_bits(a.dsave), _bits(b.dsave.to(a.dsave.device))), (what, "dsave: bits differ")
    assert torch.equal(_bits(a.ln_part), _bits(b.ln_part.to(a.ln_part.device))), (what, "ln_part: bits differ")


def check_same_bits(device, mp, form, rows=33):
    """three backward runs on one forward: identical bits of both arenas, dsave and ln_part; the poisoned twin: the clean case's
    bits, everything finite; IPLAN_AC_WGRAD_SERIAL=1 (the critic's wgrad jobs on the caller's stream): the side-stream run's bits;
    the environments reversed: every row's dsave bits move with the row, the weight gradients meet the rule (their summation order
    changed)"""
    case = case_of(f"rows{rows}", device)
    nA, E, S = case.dims[:3]
    mp.delenv("IPLAN_AC_WGRAD_SERIAL", raising=False)
    first = run_backward(case, form, mp)
    for _ in range(2):
        _same(run_backward(case, form, mp, fwd=first.fwd), first, (form, "repeat"))
    dirty = case_of(f"rows{rows}", device, poison=True)
    assert torch.isnan(dirty.buf["history"]).any() and dirty is not case
    twin = run_backward(dirty, form, mp)
    for t in twin.grads + [twin.dsave, twin.ln_part]:
        assert torch.isfinite(t).all(), (form, "the poisoned twin is not finite")
    _same(twin, first, (form, "read something outside its views"))
    mp.setenv("IPLAN_AC_WGRAD_SERIAL", "1")
    _same(run_backward(case, form, mp), first, (form, "serial wgrad jobs against the side stream"))
    mp.delenv("IPLAN_AC_WGRAD_SERIAL")
    worst = {}
    per_env = lambda t: t.reshape(2, nA, E, S, -1)  # noqa: E731
    try:
        order = list(range(E - 1, -1, -1))
        case.upload(order)
        rev = run_backward(case, form, mp)
        assert torch.equal(_bits(per_env(rev.dsave)), _bits(per_env(first.dsave)[:, :, order])), (form, "a row's dsave bits did not move with the row")
        compare_grads(rev, worst, (form, "environments reversed"))
    finally:
        case.upload()
    return worst


# ------------------------------------------------------------------------------------------------ 6: re-chunked replays
def _replay(lib, device, a, entry, what):
    for name in (entry, "iplan_ac_bwd_fc1_finalize"):
        rc = getattr(lib.c, name)(C.byref(a), _stream(device))
        assert rc == 0, (what, name, lib.c.iplan_last_error().decode())
    _sync(device)


def check_rechunk(device, mp, form, rows):
    """after a normal ops.ac_backward (which leaves dsave and the fc1.bias gradients in place) the fc1 contraction and its finalize are
    called directly on a sentinel-fenced g_part of their own with other chunkings -- fp32: 16, 32, 48 rows per chunk (at 33 rows: 3, 2
    and 1 chunks, last chunks of one row); split: 32, 64 -- and with one chunk more than needed, wholly past the rows.  Each time the
    three tensors of the finalize (sentinel-filled first) meet the rule against fp64 and the fence is intact; the replays read dsave
    from a copy with NaN in front of and behind it, so a row read past the last one shows.  The fp32 kernel returns
    early on a surplus chunk, so g_part is zero-filled for it: that form relies on the caller never passing one (the finalize sums
    every chunk); the split kernel writes the surplus chunk's zeros itself"""
    case = case_of(f"rows{rows}", device)
    lib = ops._lib(None)
    nA = case.dims[0]
    split = form == "pre"
    run = run_backward(case, form, mp)
    entry = "iplan_ac_bwd_fc1_split" if split else "iplan_ac_bwd_fc1"
    kpad = int(lib.c.iplan_ac_kpad(C.byref(run.args.fwd.feat)))
    arenas = (case.mac.actor_arena, case.mac.critic_arena)
    worst = {}
    plans = [(cr, (rows + cr - 1) // cr, False) for cr in ((32, 64) if split else (16, 32, 48))]
    plans.append((plans[-1][0], plans[-1][1] + 1, True))
    # dsave as the contraction reads it: a copy with NaN on either side (the 32-row steps of the split kernel reach past the last row)
    n = run.dsave.numel()
    poisoned = torch.full((n + 2 * POISON,), float("nan"), device=device)
    poisoned[POISON:POISON + n] = run.dsave.reshape(-1)
    for cr, chunks, surplus in plans:
        fenced = _fenced(2 * nA * chunks * M * kpad, device)
        if surplus and not split:
            fenced[2].zero_()
        a = _copy_args(run.args)
        a.dsave = poisoned[POISON:].data_ptr()
        a.g_part, a.fc1_chunk_rows, a.fc1_chunks = fenced[2].data_ptr(), cr, chunks
        for arena in arenas:
            for o, n in arena.ranges(FC1_TENSORS):
                arena.grad[:, o:o + n] = 3.25
        what = (form, rows, "chunk rows", cr, "chunks", chunks)
        _replay(lib, device, a, entry, what)
        _fence_intact(fenced, what)
        w = {}
        compare_grads(run, w, what, names=FC1_TENSORS, grads=[ar.grad.cpu() for ar in arenas])
        for k, v in w.items():
            _worse(worst, k, v)
    return worst


# ------------------------------------------------------------------------------------------------ 7: refusals
def _set(a, k, v):
    obj, name = (a, k) if "." not in k else (getattr(a, k.split(".")[0]), k.split(".")[1])
    setattr(obj, name, v)


def check_refusals(device, mp, rows=33):
    """every condition of check_bwd_args, of iplan_ac_bwd_tail / _fc1 / _fc1_finalize and of iplan_ac_bwd_fc1_split: IPLAN_EINVAL, a
    message naming the entry point, and sentinel-filled dsave / ln_part / g_part / gradient arenas untouched; a normal backward
    afterwards gives the bits of the one before"""
    case = case_of(f"rows{rows}", device)
    lib = ops._lib(None)
    EINVAL = PC._codes()
    nA = case.dims[0]
    tiles = (rows + 15) // 16
    arenas = (case.mac.actor_arena, case.mac.critic_arena)
    good = {form: run_backward(case, form, mp) for form in ("stream", "pre")}
    count = 0
    common = [{"fwd.which": 3}, {"fwd.which": -1}, {"fwd.n_agents": 0}, {"fwd.rows": 0}, {"fwd.saved": None}, {"dsave": None}, {"fwd.mode": 0},
              {"fwd.actions_in": None}, {"g_logp": None}, {"g_values": None}]
    table = {
        "iplan_ac_bwd_tail": ("stream", common + [{"ln_part": None}]),
        "iplan_ac_bwd_fc1": ("stream", common + [{"g_part": None}, {"fc1_chunk_rows": 0, "fc1_chunks": 64}, {"fc1_chunk_rows": 8, "fc1_chunks": 64},
                                                 {"fc1_chunk_rows": 24, "fc1_chunks": 64}, {"fc1_chunk_rows": 16, "fc1_chunks": (rows - 1) // 16}]),
        "iplan_ac_bwd_fc1_finalize": ("stream", common + [{"g_part": None}, {"actor_grad": None}, {"critic_grad": None}]),
        "iplan_ac_bwd_fc1_split": ("pre", [{"xb": None}, {"dsave": None}, {"g_part": None}, {"fwd.which": 0}, {"fwd.which": 1}, {"fwd.n_agents": 0},
                                           {"fwd.rows": 0}, {"fc1_chunk_rows": 16, "fc1_chunks": 64}, {"fc1_chunk_rows": 48, "fc1_chunks": 64},
                                           {"fc1_chunk_rows": 0, "fc1_chunks": 64}, {"fc1_chunk_rows": 32, "fc1_chunks": (rows - 1) // 32}]),
    }
    for entry, (form, cases) in table.items():
        base = good[form].args
        kpad = int(lib.c.iplan_ac_kpad(C.byref(base.fwd.feat)))
        bufs = [_sentinel(n, device) for n in (2 * nA * rows * L.AC_DSAVE_FLOATS, 2 * nA * tiles * L.AC_LNPART_FLOATS, 2 * nA * 64 * M * kpad)]
        sent = [b.cpu() for b in bufs]
        for fields in cases:
            a = _copy_args(base)
            a.dsave, a.ln_part, a.g_part = (b.data_ptr() for b in bufs)
            for arena in arenas:
                arena.grad.copy_(_sentinel(arena.grad.numel(), "cpu").view(arena.grad.shape))
            for k, v in fields.items():
                _set(a, k, v)
            rc = getattr(lib.c, entry)(C.byref(a), _stream(device))
            msg = lib.c.iplan_last_error().decode()
            _sync(device)
            assert rc == EINVAL and entry in msg, (entry, fields, rc, msg)
            for b, s in zip(bufs, sent):
                assert torch.equal(_bits(b.cpu()), _bits(s)), (entry, fields, "a refused call wrote a row buffer")
            for arena in arenas:
                assert torch.equal(_bits(arena.grad.cpu()), _bits(_sentinel(arena.grad.numel(), "cpu").view(arena.grad.shape))), \
                    (entry, fields, "a refused call wrote a gradient")
            count += 1
    for form, before in good.items():
        _same(run_backward(case, form, mp), before, (form, "after the refusals"))
    return {"refused": float(count)}
