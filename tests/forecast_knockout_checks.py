"""TEST INFRASTRUCTURE: forecasts under occlusion through time (csrc/predict_knockout.hip, ops.predict_knockout,
Prediction_policy.attention_knockout_trace(forecast=True)) on whatever library is active -- the host emulator in
tests/test_emu_forecast_knockout.py, the gfx950 build in tests/test_gpu_forecast_knockout.py.

The references of the bit-for-bit checks are the existing pieces: ops.predict on the same latent rows and in-place start states for the
forecasts, and the plain fp32 torch loop over ``pos`` in order for the two sums of squares (every difference, product and sum a rounded
fp32 operation of its own).  Ground truth of the values: oracle.prediction_decoder_forward in fp64 on the kernel's own latent_ko rows
(so no GAT gate flip can enter); error = max|got - ref64| / max|ref64| per net tensor (oracle_checks._grad_err), bound max(1e-5,
E32_FACTOR x the fp32 oracle's own error on the same tensor).  The sums are not compared with fp64 a second time: they are fixed, bit
for bit, by the forecasts and the host loop.  The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors."""
import functools

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.attention_checks import _codes
from tests.attention_knockout_trace_checks import _method_inputs
from tests.knockout_checks import bits, same_bits
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log
from tests.predict_checks import _e2e_args, _gumbel, _sync, _worse

A = 32
TOL = 1e-5
OUTPUTS = ops.PREDICT_KNOCKOUT_OUTPUTS
SENTINEL = -7.25

# (n_nets, B, J, H, N, P, d, pos, S, start).  Rows per net B J H N in {2, 15, 16, 17, 65, 257} (below, at and one past a tile, five tiles,
# more than one workgroup) and 102 / 12; N in {2, 5, 13, 17, 257} (15, 65 and 257 rows need an N beside 2 and 17); P in {1, 5}; d in {5, 8,
# 12} (d = 5: unaligned rows); pos reversed, across a lane-group boundary, over three groups; one net and five; H in {1, 3}, and (S, start)
# such that the last window steps have 0, 1 and P target steps left (per case below).
KERNEL_CASES = [
    (1, 1, 1, 1, 2, 1, 5, (1, 2), 3, 0),               # 2 rows; P = 1 target left
    (1, 1, 1, 3, 5, 5, 5, (2, 1), 4, 1),               # 15 rows; 2, 1, 0 targets left
    (5, 2, 2, 2, 2, 5, 8, (3, 4), 9, 1),               # 16 rows; all P targets everywhere; a lane-group boundary
    (1, 1, 1, 1, 17, 5, 12, (4, 1, 11), 2, 1),         # 17 rows; no target at all; three lane groups
    (1, 1, 5, 1, 13, 1, 5, (0,), 3, 1),                # 65 rows; 1 = P target
    (1, 1, 1, 1, 257, 5, 5, (1, 2), 3, 0),             # 257 rows: a second workgroup; 2 of 5 targets
    (5, 1, 2, 3, 17, 1, 12, (4, 1, 11), 4, 1),         # 102 rows; 1, 1, 0 targets left
    (1, 2, 1, 3, 2, 5, 8, (2, 1), 7, 0),               # 12 rows; P, P, 4 targets left
]


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def host_sq(y, ref, pos):
    """sum over ``pos`` in order of (y[c] - ref[c])^2 over the last dim, every operation a rounded fp32 operation of its own (CPU)"""
    y, ref = y.cpu(), ref.cpu()
    acc = None
    for c in pos:
        df = y[..., c] - ref[..., c]
        sq = df * df
        acc = sq if acc is None else acc + sq
    return acc


def _padded(t, lead, front, back, device, fill=float("nan")):
    """t [*dims, inner...] with ``lead`` leading dims -> (buffer, view of t's shape) on the device: the leading dims are stored in
    REVERSED order with ``front`` / ``back`` fill floats around every leading index's block, so every leading stride is larger than the
    packed one and the net stride is the smallest"""
    shape = tuple(t.shape)
    inner = int(np.prod(shape[lead:]))
    rev = tuple(reversed(shape[:lead]))
    buf = torch.full(rev + (front + inner + back,), fill, dtype=torch.float32)
    buf[..., front:front + inner] = t.permute(*reversed(range(lead)), *range(lead, t.dim())).reshape(rev + (inner,))
    buf = buf.to(device)
    view = buf[..., front:front + inner].unflatten(-1, shape[lead:]).permute(*reversed(range(lead)), *range(lead, t.dim()))
    assert view.shape == shape
    return buf, view


class Case:
    """random decoder parameters; history [n, B, S, N, d] with entity stride d + 3, latent_ko [n, B, J, H, N, 32] and pred_base [n, B, H,
    N, P, d] as strided views into NaN-filled buffers (every net, env, job and step stride larger than the packed one); the outputs
    are views into sentinel-filled buffers of the same kind"""

    def __init__(self, n, B, J, H, N, P, d, pos, S, start, device, seed=0):
        from iplan_amd.arena import ParamArena
        from iplan_amd.nova.prediction_net import Prediction_Decoder
        self.dims = (n, B, J, H, N, P, d)
        self.pos, self.S, self.start, self.device = tuple(pos), S, start, device
        assert start + H <= S
        torch.manual_seed(7 + 1000 * n + 100 * B + 10 * J + H + N + P + d + seed)
        self.mods = [Prediction_Decoder(input_size=d, hidden_size=A, output_size=d, num_layers=1, pred_length=P, teacher_forcing_ratio=0,
                                        dropout=0.0) for _ in range(n)]
        self.params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.mods]
        self.arena = ParamArena(self.mods, device)
        gen = torch.Generator().manual_seed(seed + 3 * n + 5 * B + 7 * J + 11 * H + N + P + d)
        self.hist = torch.rand(n, B, S, N, d, generator=gen) * 2 - 1
        self.latent = torch.randn(n, B, J, H, N, A, generator=gen) * 0.5
        self.pred_base = torch.rand(n, B, H, N, P, d, generator=gen) * 2 - 1
        self.upload()

    def upload(self):
        n, B, J, H, N, P, d = self.dims
        dev = self.device
        wide = torch.full((n, B, self.S, N, d + 3), float("nan"))
        wide[..., :d] = self.hist
        self.buf_hist, v = _padded(wide, 3, 3, 2, dev)
        self.d_hist = v[..., :d]                                                    # entity stride d + 3
        self.buf_lat, self.d_latent = _padded(self.latent, 4, 8, 4, dev)           # (16-byte aligned rows, strides % 4 == 0)
        self.buf_pb, self.d_pred_base = _padded(self.pred_base, 3, 1, 2, dev)
        assert self.d_hist.stride(3) == d + 3 and self.d_latent.stride(0) % 4 == 0 and self.d_latent.data_ptr() % 16 == 0

    def dest(self, want=OUTPUTS):
        """sentinel-filled strided destinations -> (dict of buffers, dict of views)"""
        n, B, J, H, N, P, d = self.dims
        bufs, views = {}, {}
        for k in want:
            inner = (N, P, d) if k == "pred_ko" else (N, P)
            bufs[k], views[k] = _padded(torch.zeros(n, B, J, H, *inner), 4, 3, 5, self.device, fill=SENTINEL)
            views[k].fill_(float("nan"))
        return bufs, views

    def run(self, want=OUTPUTS, out=None, latent=None, pred_base=None):
        latent = self.d_latent if latent is None else latent
        pred_base = self.d_pred_base if pred_base is None else pred_base
        res = ops.predict_knockout(self.arena, self.d_hist, latent, self.start, self.dims[5], pred_base=pred_base if "fshift_sq" in want else None,
                                   pos=self.pos, want=want, out=out)
        _sync(self.device)
        return res

    def targets(self):
        """(x0 [n, B, H, N, d], target [n, B, H, N, P, d] with zeros where the step is not recorded, valid [H, P])"""
        n, B, J, H, N, P, d = self.dims
        x0 = self.hist[:, :, self.start:self.start + H]
        step = self.start + torch.arange(H)[:, None] + 1 + torch.arange(P)[None, :]
        valid = step < self.S
        tg = self.hist[:, :, step.clamp_max(self.S - 1)]                           # [n, B, H, P, N, d]
        tg = torch.where(valid[None, None, :, :, None, None], tg, torch.zeros(())).permute(0, 1, 2, 4, 3, 5)
        return x0, tg, valid

    def predict_reference(self, latent=None):
        """ops.predict on the same latent rows and in-place start states -> [n, B, J, H, N, P, d] (device)"""
        n, B, J, H, N, P, d = self.dims
        latent = self.d_latent if latent is None else latent
        J = latent.shape[2]
        hs = self.d_hist.stride()
        off = (torch.arange(n)[:, None, None, None] * hs[0] + torch.arange(B)[None, :, None, None] * hs[1] +
               (self.start + torch.arange(H))[None, None, None, :] * hs[2]).expand(n, B, J, H).reshape(n, B * J * H).to(torch.int64)
        out = ops.predict(self.arena, self.d_hist, off.contiguous().to(self.device), hs[3], 0, latent.reshape(n, B * J * H * N, A).contiguous(),
                          N, P, d)
        _sync(self.device)
        return out["pred"].view(n, B, J, H, N, P, d)

    def oracle(self, dtype):
        """oracle.prediction_decoder_forward on the same rows in ``dtype`` -> [n, B, J, H, N, P, d]"""
        n, B, J, H, N, P, d = self.dims
        x0 = self.hist[:, :, None, self.start:self.start + H].expand(n, B, J, H, N, d).to(dtype)
        out = []
        for i in range(n):
            p = {k: v.to(dtype) for k, v in self.params[i].items()}
            pr = O.prediction_decoder_forward(p, x0[i].reshape(B * J * H, N, 1, d), self.latent[i].reshape(B * J * H * N, A).to(dtype), P)
            out.append(pr.reshape(B, J, H, N, P, d))
        return torch.stack(out)


@functools.lru_cache(maxsize=None)
def get_case(device, *spec):
    return Case(*spec, device)


@functools.lru_cache(maxsize=None)
def oracles(device, *spec):
    """the fp64 and fp32 oracle forecasts of a case: computed once, shared, never written"""
    case = get_case(device, *spec)
    return case.oracle(torch.float64), case.oracle(torch.float32)


# ------------------------------------------------------------------------------------------------ 1: bit for bit, and ownership
def check_kernel(device, *spec):
    """all three outputs of one launch: pred_ko = ops.predict's bits, the sums = the host loops' bits, +0.0 where no target exists, and
    nothing outside the owned elements is written"""
    case = get_case(device, *spec)
    n, B, J, H, N, P, d = case.dims
    bufs, views = case.dest()
    guards = {k: b.clone() for k, b in bufs.items()}
    operands = {k: getattr(case, k).clone() for k in ("buf_hist", "buf_lat", "buf_pb")}
    res = case.run(out=views)
    for k in OUTPUTS:
        assert res[k] is views[k] and torch.isfinite(views[k]).all(), (k, "not every owned element was written")
        own = torch.zeros_like(bufs[k], dtype=torch.bool)
        own_view = own[..., 3:3 + views[k][0, 0, 0, 0].numel()]
        own_view.fill_(True)
        assert torch.equal(bits(torch.where(own, guards[k], bufs[k])), bits(guards[k])), (k, "wrote outside what it owns")
    for k, v in operands.items():
        assert torch.equal(bits(getattr(case, k).nan_to_num(7.0)), bits(v.nan_to_num(7.0))), (k, "an operand was written")
    ref = case.predict_reference()
    assert same_bits(views["pred_ko"], ref), "pred_ko != ops.predict on the same rows"
    pk = views["pred_ko"].cpu()
    fs = host_sq(pk, case.pred_base[:, :, None].expand_as(pk), case.pos)
    assert same_bits(views["fshift_sq"].cpu(), fs), "fshift_sq != the fp32 host loop"
    _, tg, valid = case.targets()
    fe = host_sq(pk, tg[:, :, None].expand_as(pk), case.pos)
    fe = torch.where(valid[None, None, None, :, None, :], fe, torch.zeros(()))
    assert same_bits(views["ferr_sq"].cpu(), fe), "ferr_sq != the fp32 host loop against the shifted history"
    missing = views["ferr_sq"].cpu().permute(3, 5, 0, 1, 2, 4)[~valid]
    assert (bits(missing) == 0).all(), "an entry without a target is not +0.0"
    return {"fshift_sq_max": float(fs.max()), "ferr_sq_max": float(fe.max()), "targets_missing": int((~valid).sum())}


# ------------------------------------------------------------------------------------------------ 2: against fp64
def check_vs_fp64(device, *spec):
    case = get_case(device, *spec)
    r64, r32 = oracles(device, *spec)
    got = case.run(want=("pred_ko",))["pred_ko"].cpu()
    worst = {}
    for i in range(case.dims[0]):
        e32, err = _grad_err(r32[i], r64[i]), _grad_err(got[i], r64[i])
        print("predict_knockout", spec, "net", i, "pred_ko err", err, "e32", e32, "bound", _bound(e32))
        _worse(worst, "pred_ko", err)
        _worse(worst, "pred_ko_e32", e32)
        assert err <= _bound(e32), (spec, i, err, e32)
    return worst


# ------------------------------------------------------------------------------------------------ 3: independence
def check_independence(device, reps=2):
    """the same row in another tile or lane, with other jobs around it, with other outputs asked for, or with a shorter H gives the same
    bits; ``reps`` launches give the same bits"""
    spec = (2, 2, 3, 3, 5, 5, 5, (2, 1), 5, 1)
    case = Case(*spec, device, seed=3)
    full = {k: v.clone() for k, v in case.run().items() if k in OUTPUTS}
    for _ in range(reps - 1):
        again = case.run()
        for k in OUTPUTS:
            assert same_bits(again[k], full[k]), (k, "two launches differ")
    for want in (("fshift_sq",), ("ferr_sq",), ("pred_ko",), ("ferr_sq", "pred_ko")):
        part = case.run(want=want)
        assert set(k for k in part if k in OUTPUTS) == set(want)
        for k in want:
            assert same_bits(part[k], full[k]), (k, want, "depends on the other outputs asked for")
    perm = [2, 0, 1]
    moved = case.run(latent=case.d_latent[:, :, perm])
    for k in OUTPUTS:
        assert same_bits(moved[k], full[k][:, :, perm]), (k, "depends on the job's slot")
    alone = case.run(latent=case.d_latent[:, :, 1:2])
    for k in OUTPUTS:
        assert same_bits(alone[k], full[k][:, :, 1:2]), (k, "depends on the jobs around it")
    one_env = Case(*spec, device, seed=3)
    one_env.d_hist, one_env.d_latent, one_env.d_pred_base = case.d_hist[:, 1:], case.d_latent[:, 1:], case.d_pred_base[:, 1:]
    one_env.dims = (2, 1, 3, 3, 5, 5, 5)
    sub = one_env.run()
    for k in OUTPUTS:
        assert same_bits(sub[k], full[k][:, 1:]), (k, "depends on the environments around it")
    short = case.run(latent=case.d_latent[:, :, :, :2], pred_base=case.d_pred_base[:, :, :2])
    for k in OUTPUTS:
        assert same_bits(short[k], full[k][:, :, :, :2]), (k, "a shorter window is not a prefix")
    return {}


# ------------------------------------------------------------------------------------------------ 4: refusals (entry point and op)
def check_bad_arguments(device):
    """each of these is refused with its code and a message, without a launch; the op refuses on the host"""
    case = Case(1, 2, 2, 2, 5, 3, 5, (1, 2), 4, 1, device, seed=5)
    good = case.run()
    lib = ops._lib(None)
    a, _, keep = ops.predict_knockout_args(case.arena, case.d_hist, case.d_latent, case.start, 3, pred_base=case.d_pred_base, pos=case.pos,
                                           want=OUTPUTS, out={k: good[k] for k in OUTPUTS})
    EINVAL, EALIGN = _codes()

    def refused(code, **fields):
        def enter(values):
            for k, v in values.items():
                if k == "pos":
                    for i, c in enumerate(v):
                        a.pos[i] = c
                else:
                    setattr(a, k, v)
        saved = {k: (list(a.pos) if k == "pos" else getattr(a, k)) for k in fields}
        enter(fields)
        rc = lib.c.iplan_predict_knockout(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        enter(saved)
        assert rc == code and "iplan_predict_knockout" in msg, (fields, rc, msg)

    rc = lib.c.iplan_predict_knockout(None, L.C.c_void_p(0))
    assert rc == EINVAL and "iplan_predict_knockout" in lib.c.iplan_last_error().decode()
    for name in ("history", "latent_ko", "params"):
        refused(EINVAL, **{name: None})
    refused(EINVAL, fshift_sq=None, ferr_sq=None, pred_ko=None)
    refused(EINVAL, pred_base=None)
    refused(EINVAL, d=0)
    refused(EINVAL, d=17)
    for name in ("n_nets", "B", "J", "H", "N", "P"):
        refused(EINVAL, **{name: 0})
        refused(EINVAL, **{name: -2})
    refused(EINVAL, n_nets=17)
    refused(EINVAL, start=-1)
    refused(EINVAL, B=1 << 15, J=1 << 8, H=1 << 8, N=1)                          # 2^31 rows
    refused(EINVAL, B=1 << 15, J=1 << 15, H=4, N=1)                              # 2^32 rows
    refused(EINVAL, n_pos=0)
    refused(EINVAL, n_pos=17)
    refused(EINVAL, pos=(1, 5))
    refused(EINVAL, pos=(-1, 2))
    refused(EINVAL, pos=(2, 2))
    refused(EINVAL, S=2)                                                           # ferr_sq: start + H = 3 > S
    refused(EINVAL, S=0)
    refused(EALIGN, latent_ko=case.d_latent.data_ptr() + 4)
    refused(EALIGN, lat_s_job=a.lat_s_job + 1)
    refused(EALIGN, lat_s_step=a.lat_s_step + 2)
    refused(EALIGN, lat_s_net=a.lat_s_net + 3)
    lib.call("iplan_predict_knockout", a, L.current_stream(device))                # the descriptor itself is good
    _sync(device)
    again = case.run()
    for k in OUTPUTS:
        assert same_bits(again[k], good[k]), k
    # without ferr_sq S is not read; without the sums pos is not
    a.ferr_sq, a.S = None, 0
    lib.call("iplan_predict_knockout", a, L.current_stream(device))
    a.fshift_sq, a.n_pos = None, 0
    lib.call("iplan_predict_knockout", a, L.current_stream(device))
    _sync(device)

    def op_refuses(**kw):
        args = dict(history=case.d_hist, latent_ko=case.d_latent, start=case.start, P=3, pred_base=case.d_pred_base, pos=case.pos, want=OUTPUTS)
        args.update(kw)
        try:
            ops.predict_knockout(case.arena, args.pop("history"), args.pop("latent_ko"), args.pop("start"), args.pop("P"), **args)
        except AssertionError:
            return
        raise AssertionError(f"ops.predict_knockout accepted {kw}")
    op_refuses(want=())
    op_refuses(want=("pred",))
    op_refuses(pred_base=None)
    op_refuses(pred_base=case.d_pred_base[:, :, :1])                               # another window's
    op_refuses(pos=())
    op_refuses(pos=(1, 1))
    op_refuses(pos=(5,))
    op_refuses(start=-1)
    op_refuses(start=3)                                                            # start + H > S
    op_refuses(P=0)
    op_refuses(latent_ko=case.d_latent[..., :16])
    op_refuses(latent_ko=case.d_latent[:, :, :, :, 1:])                            # another N
    op_refuses(history=case.d_hist.double())
    op_refuses(out={"fshift_sq": torch.empty(1, 2, 3, 2, 5, 3, device=device)})    # a job slot too many
    op_refuses(out={"pred_ko": torch.empty(1, 2, 2, 2, 5, 3, 8, device=device)[..., :5]})
    return {}


# ------------------------------------------------------------------------------------------------ 5: the method
WANT_ALL = ("shift", "latent_ko", "pred_ko", "forecast_error")


def host_forecast_summaries(r, hist, jobs, start, D, presence_col=0):
    """float64 numpy restatement of forecast_summary and forecast_error_summary: r's arrays in the caller's layout, hist [E,S,nA,N,d]
    -> ([nA,H,P,2], [nA,H,P,2] or None)"""
    fs = np.asarray(r["forecast_shift"], dtype=np.float64)
    hist = np.asarray(hist)
    E, H, nA, N, J, P = fs.shape
    S = hist.shape[1]
    pres = hist[..., presence_col] != 0 if presence_col >= 0 else np.ones(hist.shape[:4], dtype=bool)      # [E, S, nA, N]
    with_err = "forecast_error" in r
    eb = np.asarray(r["forecast_error"], dtype=np.float64) if with_err else None
    ek = np.asarray(r["forecast_error_ko"], dtype=np.float64) if with_err else None
    out = np.full((nA, H, P, 2), np.nan)
    out_e = np.full((nA, H, P, 2), np.nan) if with_err else None
    for a in range(nA):
        for h in range(H):
            for p in range(P):
                tot, cnt, te, ce = [0.0, 0.0], [0, 0], [0.0, 0.0], 0
                for e in range(E):
                    for i in range(N):
                        for s, j in enumerate(jobs):
                            if not (pres[e, start + h, a, i] and pres[e, start:start + D, a, j].any()):
                                continue
                            tot[int(i == j)] += fs[e, h, a, i, s, p]
                            cnt[int(i == j)] += 1
                            t = start + h + 1 + p
                            if with_err and i != j and t < S and pres[e, t, a, i]:
                                te[0] += eb[e, h, a, i, p]
                                te[1] += ek[e, h, a, i, s, p]
                                ce += 1
                for col in range(2):
                    if cnt[col]:
                        out[a, h, p, col] = tot[col] / cnt[col]
                    if with_err and ce:
                        out_e[a, h, p, col] = te[col] / ce
    return out, out_e


class _Counter:
    """counts the launches of ops.predict_knockout that produce fshift_sq while it is installed"""

    def __enter__(self):
        self.calls, self.orig = [], ops.predict_knockout

        def counted(*a, **kw):
            res = self.orig(*a, **kw)
            if "fshift_sq" in kw.get("want", ()):
                self.calls.append(tuple(res["fshift_sq"].shape[1:3]))
            return res
        ops.predict_knockout = counted
        return self

    def __exit__(self, *exc):
        ops.predict_knockout = self.orig


def check_methods(device, tmp_path, E=2, S=6, N=5):
    """attention_knockout_trace(forecast=True) on a loaded checkpoint: round trips, every result against the parts and against the
    public route without the feature, chunked == unchunked, the planted unseen vehicle, the summaries, the invariances, the default path"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device, max_vehicle_num=N)
    pol, _, _ = _loaded_policy(args, tmp_path, 23)
    nA, d, P = args.n_agents, args.obs_shape_single, args.pred_length
    hist, lat, hid0, noise = _method_inputs(args, E, S, 8)
    hist[:, :, :, 1] = 0.0                                                         # a vehicle never seen: knocking it changes nothing
    lat[:, :, :, 1] = 0.0
    dv = lambda t: t.to(device)                                                    # noqa: E731
    start, D = 1, 2
    H = S - start
    pos = (2, 1)
    nzw = noise[:, :, start:start + H].contiguous()
    kw = dict(start=start, duration=D, deterministic=False, forecast=True, pos=pos, want=WANT_ALL)
    r_np = pol.attention_knockout_trace(hist.double().numpy(), lat.numpy(), hid0.numpy(), noise=nzw.numpy(), **kw)
    with _Counter() as whole:
        r_dev = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), **kw)
    assert whole.calls == [(E, N)], whole.calls
    per_env = 4 * nA * H * (2 * N * (N - 1) + N * A + N * P * (d + 1))
    per_job = 4 * nA * H * (N + N * A + 2 * N * P + N * P * d)
    tiny = (per_env + 2 * per_job + 8) / (1 << 20)                                 # one environment and two of the five jobs per chunk
    with _Counter() as chunked:
        r_chunk = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), max_workspace_mb=tiny, **kw)
    assert E >= 2 and chunked.calls == [(1, 2), (1, 2), (1, 1)] * E, ("the tiny budget did not force environment and job chunks", chunked.calls)
    _sync(device)
    shapes = {"latent": (E, H, nA, N, A), "latent_shift": (E, H, nA, N, N), "latent_ko": (E, H, nA, N, N, A), "pred": (E, H, nA, N, P, d),
              "forecast_shift": (E, H, nA, N, N, P), "forecast_error": (E, H, nA, N, P), "forecast_error_ko": (E, H, nA, N, N, P),
              "pred_ko": (E, H, nA, N, N, P, d)}
    for k, shape in shapes.items():
        assert isinstance(r_np[k], np.ndarray) and r_np[k].shape == shape and r_np[k].dtype == np.float32, (k, r_np[k].shape)
        assert torch.is_tensor(r_dev[k]) and r_dev[k].device.type == torch.device(device).type and r_dev[k].shape == shape, k
        assert np.array_equal(r_dev[k].cpu().numpy().view(np.int32), r_np[k].view(np.int32)), (k, "numpy and device round trips differ")
        assert same_bits(r_chunk[k], r_dev[k]), (k, "chunked and unchunked calls differ")
    sums = {"summary": (nA, H, 2), "forecast_summary": (nA, H, P, 2), "forecast_error_summary": (nA, H, P, 2)}
    for r in (r_np, r_dev, r_chunk):
        assert set(r) == set(shapes) | set(sums) | {"knocked", "sources", "window", "forecast_valid"}, sorted(r)
        for k, shape in sums.items():
            assert r[k].shape == shape and r[k].dtype == np.float64 and np.array_equal(r[k], r_np[k], equal_nan=True), k
        assert r["forecast_valid"].dtype == np.bool_ and r["forecast_valid"].shape == (H, P)
    # forecast_valid at the window's end: the last step has no target, the one before it one, ...
    valid = (start + np.arange(H)[:, None] + 1 + np.arange(P)[None, :]) < S
    assert np.array_equal(r_np["forecast_valid"], valid) and not valid[H - 1].any() and valid[H - 2].sum() == 1 and valid[0].all()
    # pred = ops.predict on the window's latent
    src0 = dv(hist).permute(2, 0, 1, 3, 4)
    s = src0.stride()

    def public_predict(latent, J):                                                 # latent [nA, E, J, H, N, A] -> [nA, E, J, H, N, P, d]
        off = (torch.arange(nA)[:, None, None, None] * s[0] + torch.arange(E)[None, :, None, None] * s[1] +
               (start + torch.arange(H))[None, None, None, :] * s[2]).expand(nA, E, J, H).reshape(nA, -1).to(torch.int64).contiguous()
        out = ops.predict(pol.dec_arena, src0, dv(off), s[3], 0, latent.reshape(nA, E * J * H * N, A).contiguous(), N, P, d)["pred"]
        _sync(device)
        return out.view(nA, E, J, H, N, P, d)
    pb = public_predict(r_dev["latent"].permute(2, 0, 1, 3, 4)[:, :, None], 1)[:, :, 0]      # [nA, E, H, N, P, d]
    assert same_bits(r_dev["pred"], pb.permute(1, 2, 0, 3, 4, 5)), "pred != ops.predict on latent"
    # the public route without the feature: attention_knockout_trace(want=("latent_ko",)), ops.predict on it, the differences in torch
    old = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), start=start, duration=D, deterministic=False, want=("latent_ko",))
    assert set(old) == {"latent", "latent_ko", "knocked", "sources", "window"}, sorted(old)
    pk = public_predict(old["latent_ko"].permute(2, 0, 3, 1, 4, 5), N)             # [nA, E, J, H, N, P, d]
    assert same_bits(r_dev["pred_ko"], pk.permute(1, 3, 0, 2, 4, 5, 6)), "pred_ko != ops.predict on the public latent_ko"
    acc = None
    for c in pos:
        df = pk[..., c] - pb[:, :, None, ..., c]
        acc = df * df if acc is None else acc + df * df
    assert same_bits(r_dev["forecast_shift"], acc.sqrt().permute(1, 3, 0, 4, 2, 5)), "forecast_shift != the public route's"
    # forecast_shift and the errors: torch's sqrt (on the device the method ran on) of the fp32 host loops
    ko, base = r_dev["pred_ko"].cpu(), r_dev["pred"].cpu()                         # [E, H, nA, J, N, P, d], [E, H, nA, N, P, d]
    sq = host_sq(ko, base.unsqueeze(3).expand_as(ko), pos)                         # [E, H, nA, J, N, P]
    assert same_bits(r_dev["forecast_shift"].cpu(), sq.to(device).sqrt().cpu().transpose(3, 4)), "forecast_shift != torch's sqrt of the host loop"
    step = torch.as_tensor(np.minimum(start + np.arange(H)[:, None] + 1 + np.arange(P)[None, :], S - 1))
    tg = hist[:, step].permute(0, 1, 3, 4, 2, 5)                                   # [E, H, P, nA, N, d] -> [E, H, nA, N, P, d]
    vt = torch.as_tensor(valid)
    eb = torch.where(vt[None, :, None, None, :], host_sq(base, tg, pos), torch.zeros(()))
    ek = torch.where(vt[None, :, None, None, None, :], host_sq(ko, tg.unsqueeze(3).expand_as(ko), pos), torch.zeros(()))
    assert same_bits(r_dev["forecast_error"].cpu(), eb.to(device).sqrt().cpu()), "forecast_error != torch's sqrt of the host loop"
    assert same_bits(r_dev["forecast_error_ko"].cpu(), ek.to(device).sqrt().cpu().transpose(3, 4)), "forecast_error_ko != the host loop's"
    assert (bits(r_dev["forecast_error"].cpu()[:, ~vt.any(1)]) == 0).all() and (r_dev["forecast_error"][:, 0] > 0).any()
    # the planted unseen vehicle: exact zeros and the base error at every step and horizon, echo steps included
    fsh, fek = r_dev["forecast_shift"].cpu(), r_dev["forecast_error_ko"].cpu()
    assert (bits(fsh[..., 1, :]) == 0).all(), "knocking the vehicle never seen moved a forecast"
    assert same_bits(fek[..., 1, :], r_dev["forecast_error"].cpu()), "the unseen vehicle's knocked error is not the base error"
    assert (fsh[:, :D] > 0).any() and (fsh[:, D:] > 0).any(), "no forecast moved in the knocked steps / in the echo steps"
    # the summaries against their float64 restatement; NaN where nothing counts
    fs_ref, fe_ref = host_forecast_summaries(r_np, hist.numpy(), list(range(N)), start, D)
    assert np.allclose(r_np["forecast_summary"], fs_ref, rtol=1e-12, atol=0, equal_nan=True), (r_np["forecast_summary"], fs_ref)
    assert np.allclose(r_np["forecast_error_summary"], fe_ref, rtol=1e-12, atol=0, equal_nan=True), (r_np["forecast_error_summary"], fe_ref)
    assert np.isnan(fe_ref[:, H - 1]).all() and np.isnan(fe_ref[:, ~valid]).all() and not np.isnan(fe_ref[:, 0]).all() and not np.isnan(fs_ref).all()
    every = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), start=start, duration=D, presence_col=-1, forecast=True, want=("forecast_error",))
    fs_ref, fe_ref = host_forecast_summaries({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in every.items()}, hist.numpy(),
                                             list(range(N)), start, D, presence_col=-1)
    assert np.allclose(every["forecast_summary"], fs_ref, rtol=1e-12, atol=0) and not np.isnan(fs_ref).any()
    assert np.allclose(every["forecast_error_summary"], fe_ref, rtol=1e-12, atol=0, equal_nan=True)
    assert np.array_equal(np.isnan(fe_ref[0, :, :, 0]), ~valid)
    assert "summary" not in every and "latent_shift" not in every
    # invariances: duplicates, the job order, J and the outputs asked for do not change a slot
    ents = [3, 0, 3]
    sub = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), entities=ents, start=start, duration=D, deterministic=False,
                                       forecast=True, pos=pos, want=("forecast_error",))
    one = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), entities=[0], start=start, duration=D, deterministic=False,
                                       forecast=True, pos=pos, want=())
    assert set(one) == {"latent", "pred", "forecast_shift", "forecast_summary", "knocked", "sources", "window"}, sorted(one)
    for k in ("forecast_shift", "forecast_error_ko"):
        assert same_bits(sub[k][..., 0, :], sub[k][..., 2, :]), (k, "a duplicate entity gave other bits")
        for slot, j in enumerate(ents[:2]):
            assert same_bits(sub[k][..., slot, :], r_dev[k][..., j, :]), (k, "depends on the job list", j)
    assert same_bits(one["forecast_shift"][..., 0, :], r_dev["forecast_shift"][..., 0, :]) and same_bits(one["pred"], r_dev["pred"])
    assert same_bits(sub["forecast_error"], r_dev["forecast_error"])
    # the default path: the keys of a call without forecast, and its bits
    plain = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), start=start, duration=D, deterministic=False,
                                         want=("shift", "latent_ko", "attention_ko"))
    assert set(plain) == {"latent", "latent_shift", "latent_ko", "attention_ko", "summary", "knocked", "sources", "window"}, sorted(plain)
    for k in ("latent", "latent_shift", "latent_ko"):
        assert same_bits(plain[k], r_dev[k]), (k, "forecast=True changed a result of the default path")
    assert np.array_equal(plain["summary"], r_dev["summary"], equal_nan=True)
    return {"forecast_shift_max": float(fsh.max()), "echo_forecast_shift_max": float(fsh[:, D:].max()),
            "forecast_error_max": float(r_np["forecast_error"].max())}


def check_one_step(device, tmp_path, E=2, S=3, N=5):
    """H = 1, D = 1 with hidden0 = hidden[:, start] equals attention_knockout(forecast=True) at that step, bit for bit: zero and row
    baselines, either source, with noise given and without"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device, max_vehicle_num=N)
    pol, _, _ = _loaded_policy(args, tmp_path, 31)
    d, Z = args.obs_shape_single, args.latent_dim
    hist, lat, _, noise = _method_inputs(args, E, S, 12)
    gen = torch.Generator().manual_seed(5)
    hid = torch.randn(E, S, args.n_agents, N, A, generator=gen) * 0.1
    rows = (torch.rand(d, generator=gen) - 0.5, torch.softmax(torch.randn(Z, generator=gen), -1))
    dv = lambda t: t.to(device)                                                    # noqa: E731
    worst = {}
    for s0 in (0, S - 1):
        for sources, baseline in ((("history", "behavior"), None), (("history", "behavior"), rows), (("history",), None), (("behavior",), (None, rows[1]))):
            for with_noise in (True, False):
                nz = dv(noise[:, :, s0:s0 + 1].contiguous()) if with_noise else None
                kw = dict(sources=sources, baseline=baseline, noise=nz, deterministic=not with_noise, forecast=True, pos=(1, 2), tau=0.25)
                tr = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid[:, s0]), start=s0, duration=1, horizon=1, want=(), **kw)
                ak = pol.attention_knockout(dv(hist[:, s0:s0 + 1]), dv(lat[:, s0:s0 + 1]), dv(hid[:, s0:s0 + 1]), want=(), **kw)
                _sync(device)
                for k in ("latent", "pred", "forecast_shift"):
                    assert same_bits(tr[k], ak[k]), (k, "a window of one step differs from attention_knockout(forecast=True)", s0, sources, with_noise)
                _worse(worst, "forecast_shift_max", float(tr["forecast_shift"].max()))
    assert worst["forecast_shift_max"] > 0
    return worst


def check_nothing_touched(device, tmp_path, reps):
    """the call touches no parameter, gradient entry, optimiser state or input; in the deterministic mode no generator; ``reps`` calls agree"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device)
    pol, _, _ = _loaded_policy(args, tmp_path, 29)
    hist, lat, hid0, _ = _method_inputs(args, 2, 4, 9)
    dv = lambda t: t.to(device)                                                    # noqa: E731
    pol.gat_arena.grad.normal_()
    pol.dec_arena.grad.normal_()
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), ggat=pol.gat_arena.grad.clone(), gdec=pol.dec_arena.grad.clone(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer])
    states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, np.random.get_state()[1].copy())
    inputs = [dv(hist), dv(lat), dv(hid0)]
    copies = [t.clone() for t in inputs]
    first = pol.attention_knockout_trace(*inputs, forecast=True, want=WANT_ALL)
    for _ in range(reps - 1):
        again = pol.attention_knockout_trace(*inputs, forecast=True, want=WANT_ALL)
        for k, v in first.items():
            if torch.is_tensor(v):
                assert same_bits(again[k], v), k
            elif isinstance(v, np.ndarray):
                assert np.array_equal(again[k], v, equal_nan=v.dtype == np.float64), k
    assert torch.equal(torch.get_rng_state(), states[0]) and np.array_equal(np.random.get_state()[1], states[2])
    if states[1] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), states[1])
    for t, c in zip(inputs, copies):
        assert same_bits(t, c), "an input was written"
    assert same_bits(pol.gat_arena.data, before["gat"]) and same_bits(pol.dec_arena.data, before["dec"])
    assert same_bits(pol.gat_arena.grad, before["ggat"]) and same_bits(pol.dec_arena.grad, before["gdec"])
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"]
    own = pol.attention_knockout_trace(*inputs, deterministic=False, forecast=True)      # it draws its own noise when none is given
    assert torch.isfinite(own["forecast_shift"]).all()
    return {}


def check_learn_unaffected(device, E=2):
    """learn() with injected sel / noise / keep gives the same loss and parameters whether or not a forecast knock-out ran before it"""
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
    for with_call in (False, True):
        torch.manual_seed(31)
        np.random.seed(32)
        pol = Prediction_policy(args, _Log())
        if with_call:
            D = batch.data
            r = pol.attention_knockout_trace(D["history"][:, 1:6], D["behavior_latent"][:, :5], D["attention_latent"][:, 1], start=1, duration=1,
                                             horizon=3, forecast=True, want=("forecast_error",))
            assert torch.isfinite(r["forecast_shift"]).all() and r["forecast_shift"].shape[1] == 3 and not r["forecast_valid"].all()
        losses = pol.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), pol.gat_arena.data.clone(), pol.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


def check_method_refusals(device):
    """the new refusals of attention_knockout_trace raise ValueError before anything is launched"""
    from iplan_amd.nova.prediction_policy import Prediction_policy
    args = _e2e_args(device)
    pol = Prediction_policy(args, _Log())
    hist, lat, hid0, _ = _method_inputs(args, 1, 3, 10)
    d = args.obs_shape_single

    def refuses(**kw):
        try:
            pol.attention_knockout_trace(hist.to(device), lat.to(device), hid0.to(device), **kw)
        except ValueError:
            return
        raise AssertionError(f"attention_knockout_trace accepted {kw}")
    refuses(want=("forecast_error",))
    refuses(want=("pred_ko",))
    refuses(want=("shift", "pred_ko"), forecast=False)
    refuses(want=())
    refuses(forecast=True, want=("forecast",))
    refuses(forecast=True, pos=())
    refuses(forecast=True, pos=(1, d))
    refuses(forecast=True, pos=(-1,))
    refuses(forecast=True, pos=(1, 1))
    refuses(forecast=True, pos=(True, 2))
    refuses(forecast=True, pos=(1.0, 2))
    refuses(forecast=True, max_workspace_mb=1e-4)
    ok = pol.attention_knockout_trace(hist.to(device), lat.to(device), hid0.to(device), forecast=True, pos=[2], want=())
    assert ok["forecast_shift"].shape[-1] == args.pred_length
    return {}
