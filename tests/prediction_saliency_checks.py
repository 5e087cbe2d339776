"""TEST INFRASTRUCTURE: prediction saliency (csrc/pdec_saliency.hip, ops.pdec_saliency, Prediction_policy.prediction_saliency) on whatever
library is active -- the host emulator in tests/test_emu_prediction_saliency.py, the gfx950 build in tests/test_gpu_prediction_saliency.py.

Ground truth: fp64 torch.autograd.grad through oracle.prediction_decoder_forward on the same inputs, the ReLU of every chain step on the
branch the kernel took (its ``active`` masks) -- by wrapping torch.relu for the duration of the oracle call (the
decoder calls it once per step).  The rows of a launch are independent, so the sum over the rows of <v_row, y_p[row]> gives every row's
gradient in one backward pass per job.  Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor, bound =
max(1e-5, 1.5 x e32), e32 = the fp32 oracle's own error against fp64 on the same case and branches.
The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors it saw."""
import contextlib
import copy
import functools
import itertools
from unittest import mock

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import attention_saliency_checks as AC
from tests import predict_checks as PC
from tests.kernel_checks import _sentinel
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5
A = 32
MAX_P = L.PDEC_SAL_MAX_P
JOB_OUTS = ("state_grad", "latent_grad", "state_l1", "state_gxi", "latent_l1", "latent_gxi")
OUTS = ops.PDEC_SAL_OUTPUTS
ROWS_PER_WORKGROUP = 64          # four waves of 16 rows when a tile has one task (one job, no forward walk) and P <= 7

# (S, N, P, d, n_nets, cotangent, horizons, columns): rows S * N at the 16-row tile's edges and at the workgroup's, every width with every
# raggedness of the four-column lane groups, the shortest chains and the longest the kernel takes, one net and two
KERNEL_CASES = (
    [(1, r, 2, 5, 1, "onehot", None, (1, 2)) for r in (1, 15, 16, 17, 33)]
    + [(1, r, 2, 5, 1, "onehot", [1], (2,)) for r in (ROWS_PER_WORKGROUP - 1, ROWS_PER_WORKGROUP, ROWS_PER_WORKGROUP + 1)]
    + [(3, 5, 2, dd, 1, "onehot", None, tuple(range(dd))) for dd in (1, 4, 8)]
    + [(3, 5, 2, 16, 1, "onehot", [1], tuple(range(16))), (3, 5, 5, 16, 2, "tensor", None, None)]
    + [(1, 17, 1, 5, 2, "onehot", None, (0, 4)), (1, 17, 1, 4, 1, "tensor", None, None)]
    + [(3, 7, 5, 5, 2, "onehot", None, (1, 2)), (3, 7, 5, 5, 2, "tensor", None, None), (3, 7, 5, 5, 1, "onehot", [4], (1, 2)),
       (3, 7, 5, 5, 1, "tensor", [1, 3], None), (1, 17, 5, 5, 1, "mixed", [0, 4], (3,))]
    + [(1, 17, MAX_P, 5, 1, "mixed", [0, 13, MAX_P - 1], (2,)), (2, 9, MAX_P, 4, 2, "onehot", [MAX_P - 1], (0, 3))]
)


def case_id(c):
    S, N, P, d, n, cot, hz, cols = c
    return f"S{S}_N{N}_P{P}_d{d}_n{n}_{cot}_h{'all' if hz is None else '-'.join(map(str, hz))}_c{'v' if cols is None else '-'.join(map(str, cols))}"


_sync, _worse, _bits = AC._sync, AC._worse, AC._bits


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def make_jobs(P, cot, hz, cols):
    hz = list(range(P)) if hz is None else list(hz)
    if cot == "onehot":
        return [(p, c) for p in hz for c in cols]
    if cot == "tensor":
        return [(p, None) for p in hz]
    return [(p, c) for p in hz for c in tuple(cols) + (None,)]                  # one-hot and tensor jobs in one launch


@functools.lru_cache(maxsize=8)
def get_case(dims, device, seed=0):
    case = PC.Case(*dims, device, seed=seed)
    gen = torch.Generator().manual_seed(seed + 77)
    S, N, P, d, n = dims
    case.v = torch.randn(n, S * N, P, d, generator=gen)
    case.d_v = case.v.to(device)
    return case


def run(case, jobs, v=None, want=OUTS, out=None):
    res = ops.pdec_saliency(case.arena, case.d_buf, case.d_off, case.ent_stride, case.d_h0, case.N, case.P, case.d, jobs,
                            v=v, want=want, out=out)
    _sync(case.device)
    return res


# ------------------------------------------------------------------------------------------------ the fp64 / fp32 judge
def unpack(active):
    """int32 masks [...] -> bool [..., 32]"""
    return ((active.cpu().to(torch.int64).unsqueeze(-1) >> torch.arange(32)) & 1).bool()


@contextlib.contextmanager
def pinned_relu(masks):
    """torch.relu on the given branches: call t gets masks[t] (bool, broadcastable to its argument)"""
    calls = []

    def relu(z):
        m = masks[len(calls)]
        calls.append(1)
        return z * m.to(z.dtype)

    with mock.patch.object(torch, "relu", relu):
        yield
    assert len(calls) == len(masks), (len(calls), len(masks))


def reference_rows(p, x0, h0, P, jobs, v, active, dtype):
    """one net: p = decoder state dict, x0 [R, d], h0 [R, 32], v [R, P, d] or None, active [R, P, 32] bool -> dict of pred [R, P, d],
    state_grad [R, K, d], latent_grad [R, K, 32] and the four sums [R, K] in ``dtype``"""
    R, d = x0.shape
    p = {k: t.to(dtype) for k, t in p.items()}
    xl, hl = x0.to(dtype).clone().requires_grad_(True), h0.to(dtype).clone().requires_grad_(True)
    with pinned_relu([active[:, t, None, :] for t in range(P)]):
        pred = O.prediction_decoder_forward(p, xl.reshape(1, R, 1, d), hl, P).reshape(R, P, d)
    gs, gl = [], []
    for pp, c in jobs:
        y = pred[:, pp, c].sum() if c is not None else (v[:, pp].to(dtype) * pred[:, pp]).sum()
        gx, gh = torch.autograd.grad(y, (xl, hl), retain_graph=True)
        gs.append(gx)
        gl.append(gh)
    gs, gl = torch.stack(gs, 1), torch.stack(gl, 1)
    xd, hd = xl.detach()[:, None], hl.detach()[:, None]
    return dict(pred=pred.detach(), state_grad=gs, latent_grad=gl, state_l1=gs.abs().sum(-1), state_gxi=(gs * xd).sum(-1),
                latent_l1=gl.abs().sum(-1), latent_gxi=(gl * hd).sum(-1))


def reference(case, jobs, v, active, dtype):
    x0, _ = case.gather()
    R = case.S * case.N
    act = unpack(active)
    per = [reference_rows(case.params[n], x0[n].reshape(R, case.d), case.h0[n], case.P, jobs, None if v is None else v[n].cpu(), act[n], dtype)
           for n in range(case.n_nets)]
    return {k: torch.stack([r[k] for r in per]) for k in per[0]}


def assert_vs_fp64(got, r64, r32, worst, what, keys=JOB_OUTS + ("pred",)):
    for k in keys:
        if got.get(k) is None:
            continue
        e32, err = _grad_err(r32[k], r64[k]), _grad_err(got[k], r64[k])
        print(what, k, "err", err, "e32", e32)
        _worse(worst, k, err)
        _worse(worst, k + "_e32", e32)
        assert err <= _bound(e32), (what, k, err, e32)


# ------------------------------------------------------------------------------------------------ 1: the kernel against fp64
def check_kernel(device, S, N, P, d, n, cot, hz, cols):
    case = get_case((S, N, P, d, n), device)
    jobs = make_jobs(P, cot, hz, cols)
    v = case.d_v if cot != "onehot" else None
    got = run(case, jobs, v)
    r64, r32 = (reference(case, jobs, v, got["active"], dt) for dt in (torch.float64, torch.float32))
    worst = {}
    assert_vs_fp64(got, r64, r32, worst, case_id((S, N, P, d, n, cot, hz, cols)))
    assert r64["state_grad"].abs().max() > 0 and r64["latent_grad"].abs().max() > 0
    return worst


# ------------------------------------------------------------------------------------------------ 2: every combination of outputs
def check_output_combinations(device, S=1, N=17, P=2, d=4):
    """each of the 255 non-empty subsets of the eight outputs: what is asked for has the bits of the launch that asks for everything,
    what is not is None (and its pointer NULL); the first, a middle and the full subset also against fp64"""
    case = get_case((S, N, P, d, 1), device, 1)
    jobs = make_jobs(P, "mixed", None, (0, 3))
    full = run(case, jobs, case.d_v)
    r64, r32 = (reference(case, jobs, case.d_v, full["active"], dt) for dt in (torch.float64, torch.float32))
    worst = {}
    assert_vs_fp64(full, r64, r32, worst, "all outputs")
    for r in range(1, len(OUTS) + 1):
        for sub in itertools.combinations(OUTS, r):
            got = run(case, jobs, case.d_v, want=sub)
            for k in OUTS:
                if k in sub:
                    assert torch.equal(_bits(got[k]), _bits(full[k])), (sub, k, "depends on what else was asked for")
                else:
                    assert got[k] is None and getattr(got["_args"], k) is None, (sub, k)
    return worst


# ------------------------------------------------------------------------------------------------ 3: exact statements
def _same(a, b, what, keys=OUTS):
    for k in keys:
        if a.get(k) is not None and b.get(k) is not None:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def check_exact(device, S=9, N=5, P=5, d=5, n=2):
    case = get_case((S, N, P, d, n), device, 2)
    cols = (1, 2)
    jobs = make_jobs(P, "mixed", None, cols)
    K, per = len(jobs), len(cols) + 1
    full = run(case, jobs, case.d_v)
    # the predictions are iplan_predict's
    assert torch.equal(_bits(full["pred"]), _bits(case.run(metrics=False)["pred"])), "pred != iplan_predict's"
    _same(run(case, jobs, case.d_v), full, "a second launch")
    # the sums are the plain fp32 loops over the stored gradients, columns ascending
    x0, _ = case.gather()
    for name, inp in (("state", x0.reshape(n, S * N, 1, d)), ("latent", case.h0.reshape(n, S * N, 1, A))):
        g = full[name + "_grad"].cpu()
        l1, gx = torch.zeros(n, S * N, K), torch.zeros(n, S * N, K)
        for c in range(g.shape[-1]):
            l1 = l1 + g[..., c].abs()
            gx = gx + g[..., c] * inp[..., c]
        assert torch.equal(full[name + "_l1"].cpu(), l1), (name, "l1 is not the host sum in column order")
        assert torch.equal(full[name + "_gxi"].cpu(), gx), (name, "gxi is not the host sum in column order")
    # a job's results do not depend on the other jobs ...
    for k in (0, K // 2, K - 1):
        one = run(case, [jobs[k]], case.d_v, want=JOB_OUTS)
        _same(one, {o: full[o][:, :, k:k + 1] for o in JOB_OUTS}, f"job {jobs[k]} alone", JOB_OUTS)
    sub = [2, 4]
    part = run(case, make_jobs(P, "mixed", sub, cols), case.d_v, want=JOB_OUTS)
    idx = [p * per + j for p in sub for j in range(per)]
    _same(part, {o: full[o][:, :, idx] for o in JOB_OUTS}, "horizons [2, 4] alone", JOB_OUTS)
    # ... nor on P: horizon 2 of a P = 5 launch against a P = 3 launch on the same buffer
    short = copy.copy(case)
    short.P = 3
    j2 = make_jobs(P, "onehot", [2], cols)
    _same(run(short, j2, want=JOB_OUTS), run(case, j2, want=JOB_OUTS), "P = 3 against P = 5", JOB_OUTS)
    s_pred = run(short, [], want=("pred", "active"))
    assert torch.equal(_bits(s_pred["pred"]), _bits(full["pred"][:, :, :3])) and torch.equal(s_pred["active"], full["active"][:, :, :3])
    # a row's results do not depend on its position: the samples reversed (rows change tile), and three samples launched alone
    rev = copy.copy(case)
    rev.d_off, rev.d_h0 = case.d_off.flip(1).contiguous(), case.d_h0.view(n, S, N, A).flip(1).reshape(n, S * N, A).contiguous()
    vr = case.d_v.view(n, S, N, P, d).flip(1).reshape(n, S * N, P, d).contiguous()
    flip = lambda t: t.view(n, S, N, *t.shape[2:]).flip(1).reshape(t.shape)      # noqa: E731
    _same(run(rev, jobs, vr), {o: flip(full[o]) for o in OUTS}, "samples at other positions")
    few = copy.copy(case)
    few.S = 3
    few.d_off, few.d_h0 = case.d_off[:, 4:7].contiguous(), case.d_h0.view(n, S, N, A)[:, 4:7].reshape(n, 3 * N, A).contiguous()
    vf = case.d_v.view(n, S, N, P, d)[:, 4:7].reshape(n, 3 * N, P, d).contiguous()
    cut = lambda t: t.view(n, S, N, *t.shape[2:])[:, 4:7].reshape(n, 3 * N, *t.shape[2:])      # noqa: E731
    _same(run(few, jobs, vf), {o: cut(full[o]) for o in OUTS}, "samples 4 .. 6 alone")
    # a zero cotangent: exact zeros (of those rows, and of no other)
    vz = case.d_v.clone()
    vz[:, 7] = 0.0
    z = run(case, jobs, vz, want=JOB_OUTS)
    tens = [k for k, (_, c) in enumerate(jobs) if c is None]
    for o in JOB_OUTS:
        row = z[o][:, 7][:, tens].cpu()
        assert torch.equal(row, torch.zeros_like(row)), (o, "of a zero cotangent is not exactly 0")
        assert z[o][:, 8][:, tens].abs().max() > 0
        keep = [r for r in range(S * N) if r != 7]
        assert torch.equal(_bits(z[o][:, keep]), _bits(full[o][:, keep])), (o, "another row moved")
    return {}


# ------------------------------------------------------------------------------------------------ 4: linearity in the cotangent
def check_linearity(device, S=1, N=17, P=5, d=5, alpha=0.75, beta=-1.5):
    case = get_case((S, N, P, d, 1), device, 3)
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(case.v.shape, generator=gen)
    vs = {"v": case.v, "w": w, "mix": alpha * case.v + beta * w}
    jobs = make_jobs(P, "tensor", None, None)
    got = {k: run(case, jobs, t.to(device)) for k, t in vs.items()}
    r64, r32 = (reference(case, jobs, vs["mix"], got["mix"]["active"], dt) for dt in (torch.float64, torch.float32))
    worst = {}
    for k in ("state_grad", "latent_grad"):
        comb = alpha * got["v"][k].cpu() + beta * got["w"][k].cpu()               # the fp32 rounding of the sum is part of the statement
        err, e32 = _grad_err(comb, got["mix"][k]), _grad_err(r32[k], r64[k])
        print("linearity", k, "err", err, "e32", e32)
        _worse(worst, "linearity_" + k, err)
        assert err <= _bound(e32), (k, err, e32)
    return worst


# ------------------------------------------------------------------------------------------------ 5: ownership
def check_ownership(device, S=3, N=11, P=3, d=5, n=2):
    """33 rows: a ragged last tile.  The start rows are read in place out of a buffer that is NaN wherever no start row lies; every
    destination sits inside a sentinel-filled buffer and only the owned floats change"""
    case = get_case((S, N, P, d, n), device, 4)
    jobs = make_jobs(P, "mixed", None, (1, 2))
    K, R = len(jobs), S * N
    ref = run(case, jobs, case.d_v)
    poisoned = copy.copy(case)
    buf = torch.full_like(case.buf, float("nan"))
    idx = (case.offset[:, :, None, None] + torch.arange(N)[None, None, :, None] * case.ent_stride + torch.arange(d)).reshape(-1)
    buf[idx] = case.buf[idx]
    poisoned.d_buf = buf.to(device)
    _same(run(poisoned, jobs, case.d_v), ref, "NaN around the start rows")
    shapes = dict(state_grad=(K, d), latent_grad=(K, A), state_l1=(K,), state_gxi=(K,), latent_l1=(K,), latent_gxi=(K,), pred=(P, d), active=(P,))
    pad = 37

    def carve(k, shift):
        numel = n * R * int(np.prod(shapes[k]))
        sent = _sentinel(numel + 2 * pad) + shift
        if k == "active":
            sent = sent.view(torch.int32).clone()
        buf = sent.clone().to(device)
        return sent, buf, buf[pad:pad + numel].view(n, R, *shapes[k])

    for wanted in (OUTS, ("state_l1", "latent_gxi"), ("latent_grad", "active"), ("pred",)):
        bufs = {k: carve(k, 0.0) for k in OUTS}
        got = run(case, jobs, case.d_v, want=wanted, out={k: bufs[k][2] for k in wanted})
        for k, (sent, buf, view) in bufs.items():
            host = buf.cpu()
            if k not in wanted:
                assert torch.equal(_bits(host), _bits(sent)), (k, "was not asked for and was written")
                continue
            assert got[k].data_ptr() == view.data_ptr()
            assert torch.equal(_bits(view), _bits(ref[k])), (k, "differs inside a padded buffer")
            assert torch.equal(_bits(host[:pad]), _bits(sent[:pad])) and torch.equal(_bits(host[-pad:]), _bits(sent[-pad:])), \
                (k, "a float outside the owned view was written")
    b2 = {k: carve(k, 0.25) for k in OUTS}                                      # every owned float is written
    run(case, jobs, case.d_v, out={k: b2[k][2] for k in OUTS})
    for k in OUTS:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (k, "an owned float was left unwritten")
    return {}


# ------------------------------------------------------------------------------------------------ 6: the method
def _policy(device, seed=17, **kw):
    args, pol, gat = AC._policy(device, seed, **kw)
    dec = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in pol.pred_decoder]
    return args, pol, gat, dec


def _inputs(args, E, seed=5, presence_p=0.7):
    from iplan_amd import synth
    nA, N, d, Z, P = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim, args.pred_length
    gen = torch.Generator().manual_seed(seed)
    hist = synth.make_history(gen, (E, nA), N, d, presence_p=presence_p)
    att = torch.randn(E, nA, N, A, generator=gen) * 0.1
    lat = torch.softmax(torch.randn(E, nA, N, Z, generator=gen), -1)
    noise = AC._gumbel(gen, nA, E, N, N - 1, 2)
    tgt = torch.randn(E, nA, N, P, d, generator=gen)
    return hist, att, lat, noise, tgt


def _method_reference(dec, hist, got, hz, cols, target, dtype):
    """the decoder half of the method's result through the judge, from the method's own latent: dict of [E, nA, N, H, C, ...]"""
    E, nA, N, d = hist.shape
    P = got["pred"].shape[3]
    jobs = [(p, c) for p in hz for c in cols]
    H, C = len(hz), len(cols)
    per = []
    for i in range(nA):
        r = reference_rows(dec[i], hist[:, i].reshape(E * N, d), torch.as_tensor(got["latent"])[:, i].cpu().reshape(E * N, A), P, jobs,
                           None if target is None else target[:, i].reshape(E * N, P, d), torch.as_tensor(got["active"])[:, i].cpu().reshape(E * N, P, A), dtype)
        per.append({k: (t.view(E, N, P, d) if k == "pred" else t.view(E, N, H, C, *t.shape[2:])) for k, t in r.items()})
    return {k: torch.stack([r[k] for r in per], 1) for k in per[0]}


def horizon_l1_restated(res, hist, presence_col):
    """[nA, H, 2] float64 from the method's own state_l1 / latent_l1"""
    sl, ll = (np.asarray(torch.as_tensor(res[k]).cpu(), dtype=np.float64) for k in ("state_l1", "latent_l1"))
    E, nA, N, H, C = sl.shape
    out = np.full((nA, H, 2), np.nan)
    h = np.asarray(hist)
    for a in range(nA):
        sel = h[:, a, :, presence_col] != 0 if presence_col >= 0 else np.ones((E, N), dtype=bool)
        for j in range(H):
            if sel.any():
                out[a, j] = sl[:, a, :, j][sel].mean(), ll[:, a, :, j][sel].mean()
    return out


def check_methods(device, E=3):
    """shapes and types in both conventions, every form of horizons / columns / target, values against fp64, pred and latent bit for bit
    predict's / GAT_latent_update's, deterministic == explicit zero noise, horizon_l1 restated"""
    args, pol, gat, dec = _policy(device)
    nA, N, d, Z, P = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim, args.pred_length
    hist, att, lat, noise, tgt = _inputs(args, E)
    to = lambda t: t.to(device)                                               # noqa: E731
    worst = {}
    want = ("summary", "grad", "act")
    forms = [(dict(), list(range(P)), [1, 2], None), (dict(horizons=1, columns=[0]), [1], [0], None),
             (dict(horizons=[0, 2], columns=(4, 1, 3)), [0, 2], [4, 1, 3], None), (dict(target=to(tgt)), list(range(P)), [None], tgt),
             (dict(target=to(tgt), horizons=[P - 1], columns="ignored"), [P - 1], [None], tgt)]
    for kw, hz, cols, target in forms:
        for nz in (None, noise):
            kn = dict(kw, want=want) if nz is None else dict(kw, want=want, noise=to(nz), deterministic=False)
            res = pol.prediction_saliency(to(hist), to(att), to(lat), **kn)
            _sync(device)
            H, C = len(hz), len(cols)
            shapes = {"pred": (P, d), "latent": (A,), "state_l1": (H, C), "state_gxi": (H, C), "latent_l1": (H, C), "latent_gxi": (H, C),
                      "state_grad": (H, C, d), "latent_grad": (H, C, A), "active": (P, A)}
            assert set(res) == set(shapes) | {"horizon_l1"}, set(res) ^ set(shapes)
            for k, shape in shapes.items():
                assert torch.is_tensor(res[k]) and res[k].shape == (E, nA, N) + shape and res[k].device.type == torch.device(device).type, (k, res[k].shape)
                assert res[k].dtype == (torch.bool if k == "active" else torch.float32)
            assert isinstance(res["horizon_l1"], np.ndarray) and res["horizon_l1"].dtype == np.float64 and res["horizon_l1"].shape == (nA, H, 2)
            # bit for bit the rollout's latent and predict()'s predictions
            gz = to(nz) if nz is not None else torch.zeros(nA, E, N, N - 1, 2, device=device)
            assert torch.equal(_bits(res["latent"]), _bits(pol.GAT_latent_update(to(hist), to(att), to(lat), noise=gz))), "latent != GAT_latent_update's"
            assert torch.equal(_bits(res["pred"]), _bits(pol.predict(to(hist), to(att), to(lat), noise=gz))), "pred != predict()'s"
            r64, r32 = (_method_reference(dec, hist, res, hz, cols, target, dt) for dt in (torch.float64, torch.float32))
            assert_vs_fp64(res, r64, r32, worst, f"method {sorted(kw)}")
            np.testing.assert_allclose(res["horizon_l1"], horizon_l1_restated(res, hist, 0), rtol=1e-12, atol=0)
            if nz is None:
                zero = pol.prediction_saliency(to(hist), to(att), to(lat), **dict(kn, noise=torch.zeros_like(noise).to(device), deterministic=False))
                for k in shapes:
                    assert torch.equal(_bits(zero[k]), _bits(res[k])), (k, "deterministic != explicit zero noise")
            few = pol.prediction_saliency(to(hist), to(att), to(lat), **dict(kn, want=()))
            assert set(few) == {"pred", "latent", "horizon_l1"}
            assert torch.equal(_bits(few["pred"]), _bits(res["pred"])) and np.array_equal(few["horizon_l1"], res["horizon_l1"], equal_nan=True)
    # numpy in -> numpy out (float64 histories, as the runner hands them over)
    res_np = pol.prediction_saliency(hist.double().numpy(), att.numpy(), lat.numpy(), target=tgt.numpy(), want=want)
    res_t = pol.prediction_saliency(to(hist), to(att), to(lat), target=to(tgt), want=want)
    for k in res_t:
        assert isinstance(res_np[k], np.ndarray), k
        assert np.array_equal(res_np[k], res_t[k] if k == "horizon_l1" else res_t[k].cpu().numpy(), equal_nan=True), k
    # horizon_l1: presence_col < 0 counts every row, another column changes the rows, nothing present gives NaN (of that agent only)
    base = pol.prediction_saliency(to(hist), to(att), to(lat))
    assert (hist[..., 0] == 0).any() and np.isfinite(base["horizon_l1"]).all()
    r = pol.prediction_saliency(to(hist), to(att), to(lat), presence_col=-1)
    np.testing.assert_allclose(r["horizon_l1"], horizon_l1_restated(r, hist, -1), rtol=1e-12, atol=0)
    assert not np.array_equal(r["horizon_l1"], base["horizon_l1"]), "presence_col = -1 did not count the absent rows"
    h3 = hist.clone()
    h3[:, :, 1, 3] = 0.0                                                       # entity 1 is absent by column 3 alone
    r = pol.prediction_saliency(to(h3), to(att), to(lat), presence_col=3)
    np.testing.assert_allclose(r["horizon_l1"], horizon_l1_restated(r, h3, 3), rtol=1e-12, atol=0)
    assert not np.array_equal(r["horizon_l1"], pol.prediction_saliency(to(h3), to(att), to(lat))["horizon_l1"])
    gone = hist.clone()
    gone[:, 0, :, 0] = 0.0
    r = pol.prediction_saliency(to(gone), to(att), to(lat))
    assert np.isnan(r["horizon_l1"][0]).all() and np.isfinite(r["horizon_l1"][1]).all()
    np.testing.assert_allclose(r["horizon_l1"], horizon_l1_restated(r, gone, 0), rtol=1e-12, atol=0, equal_nan=True)
    # its own noise: finite, and drawn from the generator
    state = torch.get_rng_state()
    own = pol.prediction_saliency(to(hist), to(att), to(lat), deterministic=False)
    assert torch.isfinite(own["state_l1"]).all()
    if torch.device(device).type == "cpu":
        assert not torch.equal(torch.get_rng_state(), state)
    return worst


# ------------------------------------------------------------------------------------------------ 7: the chain through the GAT
def check_chain(device, dims=(2, 1, 2, 3, 5)):
    """social=(p, c): input_grad against fp64 autograd of sum_i pred[i, p, c] through oracle.gat_forward + oracle.prediction_decoder_forward
    with respect to [history || behavior_latent] of all entities, on the kernels' own ReLU branches; pair_gxi summed over the egos
    against the GAT part; chunked == unchunked.  tau is the policy's own launch value, so the oracle is run at tau 1 and 0.25 by patching
    ops.gat_forward's default"""
    nA, E, _, N, d = dims
    E = max(E, 2)
    args, pol, gat, dec = _policy(device, 23, max_vehicle_num=N, n_agents=nA)
    Z, P = args.latent_dim, args.pred_length
    hist, att, lat, noise, tgt = _inputs(args, E, seed=8, presence_p=2.0)
    to = lambda t: t.to(device)                                               # noqa: E731
    worst = {}
    real_forward = ops.gat_forward
    for tau, social, kw in ((1.0, (P - 1, 2), dict()), (0.25, (0, 1), dict()), (0.25, 1, dict(target=to(tgt))), (1.0, (1, 1), dict(gate="held"))):
        with mock.patch.object(ops, "gat_forward", lambda *a, **k: real_forward(*a, **dict(k, tau=tau))):
            res = pol.prediction_saliency(to(hist), to(att), to(lat), social=social, want=("grad", "act"), **kw)
            small = pol.prediction_saliency(to(hist), to(att), to(lat), social=social, want=("grad", "act"), max_workspace_mb=0.1, **kw)
            sal = pol.attention_saliency(to(hist).unsqueeze(1), to(lat).unsqueeze(1), hidden=to(att).unsqueeze(1), tau=tau, want=(),
                                         target=0, gate=kw.get("gate", "through"))
        _sync(device)
        assert set(small) == set(res)
        for k in res:
            if k != "horizon_l1":
                assert torch.equal(_bits(small[k]), _bits(res[k])), (k, "chunked differs from unchunked")
        assert res["pair_gl1"].shape == (E, nA, N, N, 2) and res["pair_gxi"].shape == (E, nA, N, N, 2) and res["input_grad"].shape == (E, nA, N, d + Z)
        held = kw.get("gate") == "held"
        tensor = "target" in kw
        p_job = social if tensor else social[0]
        hz = list(range(P))
        k_h = hz.index(p_job)
        k_c = 0 if tensor else [1, 2].index(social[1])
        ah, av = sal["active_h"][:, 0].cpu(), sal["active_v"][:, 0].cpu()
        act = res["active"].cpu()
        refs = {}
        for dt in (torch.float64, torch.float32):
            total, gat_part = torch.zeros(E, nA, N, d + Z, dtype=dt), torch.zeros(E, nA, N, d + Z, dtype=dt)
            for i in range(nA):
                h_leaf, b_leaf = hist[:, i].to(dt).clone().requires_grad_(True), lat[:, i].to(dt).clone().requires_grad_(True)
                obs = torch.cat([h_leaf, b_leaf], -1)
                g = {k: t.to(dt) for k, t in gat[i].items()}
                with AC._pinned(ah[:, i], av[:, i], held):
                    h0 = O.gat_forward(g, obs, att[:, i].to(dt).reshape(E * N, A), torch.zeros(E * N * (N - 1), 2, dtype=dt), tau=tau)
                dd = {k: t.to(dt) for k, t in dec[i].items()}
                outs = []
                for x0, direct in ((h_leaf, True), (h_leaf.detach(), False)):        # the whole chain, and its GAT path alone
                    with pinned_relu([act[:, i, :, t].reshape(E * N, 1, A) for t in range(P)]):
                        pred = O.prediction_decoder_forward(dd, x0.reshape(E, N, 1, d), h0, P)
                    y = (tgt[:, i, :, p_job].to(dt) * pred[:, :, p_job]).sum() if tensor else pred[:, :, p_job, social[1]].sum()
                    outs.append(torch.cat(torch.autograd.grad(y, (h_leaf, b_leaf), retain_graph=True), -1))
                total[:, i], gat_part[:, i] = outs
            refs[dt] = (total, gat_part)
        (t64, g64), (t32, g32) = refs[torch.float64], refs[torch.float32]
        e32, err = _grad_err(t32, t64), _grad_err(res["input_grad"], t64)
        # pair_gxi summed over the egos and the sources = <GAT part of input_grad, inputs>, per entity
        obs = torch.cat([hist, lat], -1)
        px = res["pair_gxi"].double().cpu().sum((2, 4))
        px64, px32 = (g64 * obs).sum(-1), (g32.double() * obs).sum(-1)
        e32p, errp = _grad_err(px32, px64), _grad_err(px, px64)
        direct = _grad_err(res["state_grad"][:, :, :, k_h, k_c].cpu(), (t64 - g64)[..., :d])
        e32d = _grad_err((t32 - g32)[..., :d], (t64 - g64)[..., :d])
        print("chain tau", tau, social, sorted(kw), "input_grad err", err, "e32", e32, "pair_gxi err", errp, "e32", e32p, "direct", direct,
              "share of the GAT path", g64.abs().max().item() / t64.abs().max().item())
        _worse(worst, "chain_input_grad", err)
        _worse(worst, "chain_input_grad_e32", e32)
        _worse(worst, "chain_pair_gxi", errp)
        _worse(worst, "chain_pair_gxi_e32", e32p)
        assert g64.abs().max() > 0 and (t64 - g64).abs().max() > 0
        assert err <= _bound(e32), ("input_grad", tau, social, err, e32)
        assert errp <= _bound(e32p), ("pair_gxi", tau, social, errp, e32p)
        assert direct <= _bound(e32d), ("state_grad against the direct path", tau, social, direct, e32d)
    return worst


# ------------------------------------------------------------------------------------------------ 8: touches nothing
def check_touches_nothing(device, E=2):
    from iplan_amd import synth
    from iplan_amd.nova.prediction_policy import Prediction_policy
    args, pol, _, _ = _policy(device)
    nA, N, P, S = args.n_agents, args.max_vehicle_num, args.pred_length, args.pred_batch_size
    batch = synth.make_batch(args, E, seed=9, terminated_p=0.1, device=device)
    D = batch.data
    ins = (D["history"][:, 2], D["attention_latent"][:, 2], D["behavior_latent"][:, 2])
    copies = [t.clone() for t in ins]
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), ggrad=pol.gat_arena.grad.clone(), dgrad=pol.dec_arena.grad.clone(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer], rng=torch.get_rng_state(), np=np.random.get_state()[1].copy(),
                  crng=torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, vars=sorted(vars(pol)))
    res = pol.prediction_saliency(*ins, want=("summary", "grad", "act"), social=(1, 2))
    _sync(device)
    assert torch.isfinite(res["input_grad"]).all() and torch.isfinite(res["state_grad"]).all()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, copies)), "an input was written"
    assert torch.equal(pol.gat_arena.data, before["gat"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert torch.equal(_bits(pol.gat_arena.grad), _bits(before["ggrad"])) and torch.equal(_bits(pol.dec_arena.grad), _bits(before["dgrad"]))
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"] and sorted(vars(pol)) == before["vars"]
    assert torch.equal(torch.get_rng_state(), before["rng"]) and np.array_equal(np.random.get_state()[1], before["np"])
    if before["crng"] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), before["crng"])
    # a following learn() gives the same bits with and without a preceding call
    gen = torch.Generator().manual_seed(21)
    avail = args.episode_limit - P - 1
    sel = torch.stack([torch.randperm(E * avail, generator=gen)[:S] for _ in range(nA)]).numpy()
    noise = AC._gumbel(gen, nA, S, N, N - 1, 2).to(device)
    keep = (torch.rand(nA, P, S * N, args.attention_dim, generator=gen) < 1.0 - args.decoder_dropout).float().to(device)
    results = []
    for with_call in (False, True):
        torch.manual_seed(31)
        np.random.seed(32)
        p2 = Prediction_policy(args, _Log())
        if with_call:
            p2.prediction_saliency(*ins, social=(0, 1), gate="held")
        losses = p2.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), p2.gat_arena.data.clone(), p2.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


# ------------------------------------------------------------------------------------------------ 9: refusals
def check_entry_point_refusals(device):
    """each of these is refused with IPLAN_EINVAL and a message, without a launch: the destinations keep their sentinels"""
    case = get_case((1, 17, 3, 5, 1), device, 6)
    jobs = [(0, 1), (2, None), (1, 4)]
    good = run(case, jobs, case.d_v)
    lib = ops._lib(None)
    K, R, P, d = len(jobs), 17, 3, 5
    shapes = dict(state_grad=(K, d), latent_grad=(K, A), state_l1=(K,), state_gxi=(K,), latent_l1=(K,), latent_gxi=(K,), pred=(P, d), active=(P,))
    sent = {k: (_sentinel(R * int(np.prod(s))).view(torch.int32 if k == "active" else torch.float32).clone()).view(1, R, *s) for k, s in shapes.items()}
    out = {k: t.clone().to(device) for k, t in sent.items()}
    res = run(case, jobs, case.d_v, out=out)
    for k in OUTS:
        out[k].copy_(sent[k])
    a = res["_args"]
    EINVAL, _ = AC._codes()
    host = L.C.cast(L.C.c_void_p(a.jobs_host), L.C.POINTER(L.C.c_int32))

    def untouched():
        _sync(device)
        for k in OUTS:
            assert torch.equal(_bits(out[k].cpu()), _bits(sent[k])), (k, "a refused call launched")

    def refused(job=None, **fields):
        old = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        old_job = None
        if job is not None:
            old_job = (host[2 * job[0]], host[2 * job[0] + 1])
            host[2 * job[0]], host[2 * job[0] + 1] = job[1], job[2]
        rc = lib.c.iplan_pdec_saliency(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, v in old.items():
            setattr(a, k, v)
        if old_job is not None:
            host[2 * job[0]], host[2 * job[0] + 1] = old_job
        assert rc == EINVAL and "iplan_pdec_saliency" in msg, (fields, job, rc, msg)
        untouched()

    assert lib.c.iplan_pdec_saliency(None, L.C.c_void_p(0)) == EINVAL
    for field, bad in (("n_nets", 0), ("n_nets", L.MAX_NETS + 1), ("S", 0), ("N", 0), ("P", 0), ("P", MAX_P + 1), ("d", 0), ("d", 17), ("K", -1), ("K", 0)):
        refused(**{field: bad})
    for field in ("x0", "h0", "offset", "params", "jobs", "jobs_host"):
        refused(**{field: None})
    refused(**{k: None for k in OUTS})                                         # nothing asked for
    refused(job=(0, 3, 1))                                                     # p >= P
    refused(job=(1, -1, 1))
    refused(job=(2, 1, 5))                                                     # c >= d
    refused(job=(2, 1, -2))
    refused(v=None)                                                            # job 1 takes its cotangent from v
    lib.call("iplan_pdec_saliency", a)                                         # the restored descriptor is accepted
    _sync(device)
    _same(out, good, "after the refusals")
    # the forward walk alone needs no jobs
    for k in OUTS:
        out[k].copy_(sent[k])
    saved = {k: getattr(a, k) for k in JOB_OUTS + ("jobs", "jobs_host", "v")}
    for k in saved:
        setattr(a, k, None)
    a.K = 0
    lib.call("iplan_pdec_saliency", a)
    _sync(device)
    _same(out, good, "pred and active without jobs", ("pred", "active"))
    for k in JOB_OUTS:
        assert torch.equal(_bits(out[k].cpu()), _bits(sent[k])), (k, "was written without being asked for")
    del res
    return {}


def check_method_refusals(device):
    args, pol, _, _ = _policy(device)
    nA, N, d, Z, P = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim, args.pred_length
    E = 2
    hist, att, lat = torch.rand(E, nA, N, d).to(device), torch.rand(E, nA, N, A).to(device), torch.rand(E, nA, N, Z).to(device)
    tgt = torch.zeros(E, nA, N, P, d).to(device)

    def refused(*a, exc=ValueError, pol=pol, **kw):
        try:
            pol.prediction_saliency(*a, **kw)
        except exc as e:
            assert type(e) is exc and "prediction_saliency" in str(e), e
            return
        raise AssertionError(f"not refused: {kw}")

    refused(hist, att)                                                        # behavior_latent missing
    refused(hist[0], att, lat)
    refused(hist[..., :d - 1], att, lat)
    refused(hist[:, :1], att, lat)
    refused(hist[:, :, :1], att[:, :, :1], lat[:, :, :1])                      # one entity: no GAT
    refused(hist, att[..., :A - 1], lat)
    refused(hist, att, lat[..., :Z - 1])
    refused(hist, att, lat, columns=())
    refused(hist, att, lat, columns=(1, d))
    refused(hist, att, lat, columns=(1, 1))
    refused(hist, att, lat, columns=(1.5,))
    refused(hist, att, lat, horizons=P)
    refused(hist, att, lat, horizons=[])
    refused(hist, att, lat, horizons=[1, 0])
    refused(hist, att, lat, horizons=[1, 1])
    refused(hist, att, lat, horizons=[-1])
    refused(hist, att, lat, horizons=1.0)
    refused(hist, att, lat, target=tgt[..., :d - 1])
    refused(hist, att, lat, target=tgt[:, :, :, 0])
    refused(hist, att, lat, target="self")
    refused(hist, att, lat, target=3)
    refused(hist, att, lat, noise=torch.zeros(nA, E, N, N - 1, 2))            # with deterministic=True
    refused(hist, att, lat, noise=torch.zeros(nA, E, N, N, 2), deterministic=False)
    refused(hist, att, lat, social=(P, 1))
    refused(hist, att, lat, social=(0, 3))
    refused(hist, att, lat, social=1)
    refused(hist, att, lat, horizons=[0, 2], social=(1, 1))
    refused(hist, att, lat, target=tgt, social=(1, 1))
    refused(hist, att, lat, target=tgt, horizons=[0], social=1)
    refused(hist, att, lat, gate="soft")
    refused(hist, att, lat, want=("summary", "maps"))
    refused(hist, att, lat, presence_col=d)
    refused(hist, att, lat, presence_col=0.5)
    refused(hist, att, lat, social=(0, 1), max_workspace_mb=0.001)
    long_args, long_pol, _, _ = _policy(device, pred_length=MAX_P + 1, episode_limit=MAX_P + 8)
    refused(hist, att, lat, exc=NotImplementedError, pol=long_pol)
    ok = pol.prediction_saliency(hist, att, lat, social=(0, 1), max_workspace_mb=0.3)
    assert torch.isfinite(ok["input_grad"]).all()
    return {}
