"""TEST INFRASTRUCTURE: intent knock-out through time (csrc/enc_knockout.hip, ops.enc_knockout, Behavior_policy.latent_knockout) on
whatever library is active -- the host emulator in tests/test_emu_latent_knockout.py, the gfx950 build in
tests/test_gpu_latent_knockout.py.

References: (a) bit for bit, ops.beh_eval(want_latent=True) / latent_trace on an EXPLICIT copy of the history with the job's steps and
columns replaced for all vehicles (``knocked_copy``); (b) plain fp32 host loops for the sums of squares, the argmax and the flips, and a
numpy float64 restatement of the summaries; (c) oracle.encoder_forward stepped window by window on the copy, in fp64 and fp32.
Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor (``_grad_err``),
bound = max(1e-5, E32_FACTOR x the fp32 oracle's own error against fp64 on the same inputs).  No other hand-set number.
The checks never touch ``L.use_library_for_tests``: the caller decides which library is active.  Each returns the worst errors it saw."""
import ctypes as C

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import behavior_eval_checks as BC
from tests.oracle_checks import E32_FACTOR, _grad_err

TOL = 1e-5
COEF, THRES = BC.COEF, BC.THRES
ALL = ops.ENC_KO_OUTPUTS
JOB_KEYS = ("latent_ko", "hidden_ko", "intent", "latent_shift_sq", "state_shift_sq")
ROW = "row"            # a fixed baseline row per net, drawn by the case
MAX_SKIPPED = 0.01     # share of intent / flip entries whose fp64 top-two margin is inside the bound

# (E, N, d, Z, L, J, n_nets, starts, D, H, columns, baseline): rows E * N in {1, 15, 16, 17, 33, 65} -- the 16-row tile's edges, one row
# past two tiles and one past a 4-wave workgroup; (d, Z) in {(1, 1), (5, 8), (12, 4), (8, 8)}; L in {1, 2, 3, 10}; n_nets in {1, 2, 5};
# s = 0 (zero start state, padded windows) and s = J - 1 (one valid window); D = 1, D > L, D reaching past J; H = 1, H past J; Q = 1 and
# Q = 5 with adjacent starts; column subsets; the three baselines.  J <= 12.
KERNEL_CASES = [
    (1, 1, 1, 1, 1, 1, 1, (0,), 1, 1, None, None),
    (3, 5, 5, 8, 10, 12, 2, (0, 1, 2, 3, 4), 1, 4, None, "hold"),
    (2, 8, 12, 4, 2, 6, 5, (0, 5), 3, 3, (0, 3, 11), ROW),
    (1, 17, 8, 8, 3, 7, 1, (2,), 9, 7, None, None),
    (3, 11, 5, 8, 3, 5, 1, (1, 3), 4, 1, (1, 2), "hold"),
    (5, 13, 8, 8, 2, 4, 2, (0, 3), 1, 2, (7,), ROW),
    (1, 16, 5, 8, 10, 12, 1, (3, 11), 5, 6, (0,), None),
    (1, 15, 1, 1, 2, 5, 2, (0, 2, 4), 2, 5, None, ROW),
]
# against the fp64 oracle: the same edges, fewer of them, plus d + Z > 16, which beh_eval cannot run
ORACLE_CASES = KERNEL_CASES[1:6] + [(2, 9, 12, 8, 3, 6, 2, (0, 2, 5), 2, 4, (0, 5, 11), "hold")]
# (E, N, d, Z, L, J, n_nets, starts, D, H) of the sentinel check: ragged tiles
SENTINEL_CASES = [(1, 17, 5, 8, 2, 4, 2, (1, 3), 2, 3), (3, 11, 12, 1, 3, 3, 1, (0, 2), 1, 2), (1, 2, 16, 16, 1, 2, 5, (0, 1), 3, 1)]


def _sync(device):
    BC._sync(device)


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def _bits(t):
    t = torch.as_tensor(t)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu()
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64).cpu()
    return t.cpu()


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (what, "differs bitwise", tuple(a.shape), tuple(b.shape))


def knocked_copy(hist, s, D, cols, baseline):
    """hist [n, E, T, N, d] on the host -> a copy with columns ``cols`` (None: all) of steps s .. s+D-1 replaced for every vehicle:
    baseline None = zeros, "hold" = the vehicle's own row of step s-1 (zeros when s = 0), else a row [n, d]"""
    n, E, T, N, d = hist.shape
    cols = list(range(d)) if cols is None else list(cols)
    out = hist.clone()
    hi = min(s + D, T)
    if isinstance(baseline, str):
        fill = hist[:, :, s - 1] if s > 0 else torch.zeros_like(hist[:, :, 0])          # [n, E, N, d]
        fill = fill[:, :, None].expand(n, E, hi - s, N, d)
    elif baseline is None:
        fill = torch.zeros(n, E, hi - s, N, d, dtype=hist.dtype)
    else:
        fill = baseline.to(hist.dtype)[:, None, None, None, :].expand(n, E, hi - s, N, d)
    out[:, :, s:hi, :, cols] = fill[..., cols]
    return out


class Case:
    """random encoders (and decoders, for the beh_eval reference) and the strided episode buffer of behavior_eval_checks.Case"""

    def __init__(self, E, N, d, Z, Lw, J, n_nets, device, seed=0):
        self.base = BC.Case(E, N, Lw, J, d, Z, n_nets, device, seed=seed)
        self.E, self.N, self.d, self.Z, self.L, self.J, self.n_nets, self.device = E, N, d, Z, Lw, J, n_nets, device
        self.T, self.rows = self.base.T, E * N
        self.enc_p, self.enc_arena, self.dec_arena = self.base.enc_p, self.base.enc_arena, self.base.dec_arena
        self.row = torch.rand(n_nets, d, generator=torch.Generator().manual_seed(77 + seed)) * 2 - 1
        self.hist = self.base.view(self.base.buf).contiguous()                          # [n, E, T, N, d] on the host

    @property
    def d_hist(self):
        return self.base.d_hist

    def baseline(self, b):
        return self.row if b == ROW else b

    def run(self, starts, D, H, cols=None, baseline=None, want=ALL, hist=None, out=None, workspace=None):
        kw = dict(hold=True) if baseline == "hold" else dict(baseline=None if baseline is None else self.row.to(self.device))
        res = ops.enc_knockout(self.enc_arena, self.d_hist if hist is None else hist, list(starts), D, H, self.L, self.Z, COEF, columns=cols,
                               want=want, out=out, workspace=workspace, **kw)
        _sync(self.device)
        return res

    def trace(self, hist):
        """beh_eval's latent [n, rows, J, Z] on a history [n, E, T, N, d] given on the host"""
        out = ops.beh_eval(self.enc_arena, self.dec_arena, hist.to(self.device), None, self.L, self.Z, COEF, THRES, want_latent=True,
                           want_recon=False, want_sums=False)
        _sync(self.device)
        return out["latent"].cpu()

    def copy_of(self, s, D, cols, baseline):
        return knocked_copy(self.hist, s, D, cols, self.baseline(baseline))


def windows_of(J, starts, H):
    return [[s + h for h in range(H) if s + h < J] for s in starts]


# ------------------------------------------------------------------------------------------------ 1: bit for bit against beh_eval
def check_vs_trace(device, E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline):
    """latent_ko at every reported window equals beh_eval's latent on an explicit copy, latent on [0, Jn) equals beh_eval's on the
    history itself, bit for bit; slots of windows past J are zero"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device)
    got = case.run(starts, D, H, cols, baseline)
    Jn = min(J, max(starts) + H)
    assert got["latent"].shape == (n_nets, case.rows, Jn, Z) and got["latent_ko"].shape == (n_nets, case.rows, len(starts), H, Z)
    _same(got["latent"], case.trace(case.hist)[:, :, :Jn], "the base chain vs beh_eval")
    moved = 0.0
    for q, s in enumerate(starts):
        ref = case.trace(case.copy_of(s, D, cols, baseline))
        nw = min(H, J - s)
        _same(got["latent_ko"][:, :, q, :nw], ref[:, :, s:s + nw], ("latent_ko vs beh_eval on the copy", q, s))
        for k in JOB_KEYS:
            assert not bool((got[k][:, :, q, nw:] != 0).any()), (k, "a window past J is not zero")
        moved = max(moved, float((got["latent_ko"][:, :, q, :nw].cpu() - got["latent"][:, :, s:s + nw].cpu()).abs().max()))
    assert moved > 0.0 or Z == 1, "no job moved a latent"
    return {"latent_moved_max": moved}


# ------------------------------------------------------------------------------------------------ 2: host loops
def host_shift_sq(x, base):
    """sum_c (x - base)^2, c ascending, every operation rounded to fp32 on its own: [.., C] x 2 -> [..]"""
    x, base = np.asarray(x, dtype=np.float32), np.asarray(base, dtype=np.float32)
    s = np.zeros(x.shape[:-1], dtype=np.float32)
    for c in range(x.shape[-1]):
        df = (x[..., c] - base[..., c]).astype(np.float32)
        s = (s + (df * df).astype(np.float32)).astype(np.float32)
    return s


def _dev_sqrt(sq, device):
    """torch's sqrt on the device the method forms the shifts on (a vectorised host sqrt need not round like numpy's)"""
    return torch.sqrt(torch.from_numpy(np.ascontiguousarray(sq)).to(device)).cpu().numpy()


def host_argmax(x):
    return np.argmax(np.asarray(x), axis=-1)                                            # the first of the largest: lowest index on ties


def check_host_loops(device, E=3, N=11, d=5, Z=8, Lw=3, J=7, n_nets=2, starts=(0, 2, 6), D=2, H=4, cols=(1, 3), baseline="hold"):
    """latent_shift_sq, state_shift_sq, intent and intent_base equal fp32 host loops over latent_ko / hidden_ko and the base record, bit
    for bit; hidden_ko equals he of a base walk on the copy (the op on the copy, its he record read from the workspace)"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=3)
    Jn = min(J, max(starts) + H)
    ws = torch.zeros(n_nets * case.rows * Jn * 32, device=device)
    got = case.run(starts, D, H, cols, baseline, workspace=ws)
    he = ws.cpu().reshape(n_nets, case.rows, Jn, 32).numpy()
    lat = got["latent"].cpu().numpy()
    assert np.array_equal(got["intent_base"].cpu().numpy(), host_argmax(lat))
    for q, s in enumerate(starts):
        nw = min(H, J - s)
        lk, hk = got["latent_ko"][:, :, q, :nw].cpu().numpy(), got["hidden_ko"][:, :, q, :nw].cpu().numpy()
        _same(got["latent_shift_sq"][:, :, q, :nw], torch.from_numpy(host_shift_sq(lk, lat[:, :, s:s + nw])), ("latent_shift_sq", q))
        _same(got["state_shift_sq"][:, :, q, :nw], torch.from_numpy(host_shift_sq(hk, he[:, :, s:s + nw])), ("state_shift_sq", q))
        assert np.array_equal(got["intent"][:, :, q, :nw].cpu().numpy(), host_argmax(lk)), ("intent", q)
        # he of the copy's own base chain at the job's windows
        j = s + nw - 1
        ws2 = torch.zeros(n_nets * case.rows * (j + 1) * 32, device=device)
        case.run([j], 1, 1, None, None, want=("latent",), hist=case.copy_of(s, D, cols, baseline).to(device), workspace=ws2)
        he2 = ws2.cpu().reshape(n_nets, case.rows, j + 1, 32)
        _same(got["hidden_ko"][:, :, q, :nw], he2[:, :, s:], ("hidden_ko vs the base walk on the copy", q))
    assert float(got["state_shift_sq"].max()) > 0.0 and float(got["latent_shift_sq"].max()) > 0.0
    return {"latent_shift_sq_max": float(got["latent_shift_sq"].max()), "state_shift_sq_max": float(got["state_shift_sq"].max())}


# ------------------------------------------------------------------------------------------------ 3: exact zeros
def _plus_zero(t, what):
    t = t.cpu()
    assert bool((t == 0).all()) and not bool(torch.signbit(t).any()), (what, "is not exactly +0.0")


def check_exact_zeros(device):
    """a job whose replaced values equal the originals moves nothing at any window, echo included: a planted all-zero vehicle under the
    zero baseline, and "hold" on a constant row; Z = 1 gives latent_shift = +0.0 everywhere with state_shift > 0 somewhere"""
    E, N, d, Z, Lw, J, n_nets = 2, 9, 5, 8, 3, 8, 2
    starts, D, H = (0, 2, 5), 3, 6
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=5)
    buf = case.base.buf
    hv = case.base.view(buf)                                                            # a view: writes land in the buffer
    hv[:, :, :, 4] = 0.0                                                                # vehicle 4 of every env is never seen
    hv[:, 1, 1:5, 7] = hv[:, 1, 1:2, 7]                                                 # vehicle 7 of env 1 holds its row over steps 1 .. 4
    case.base.upload()
    case.hist = hv.contiguous()
    zero = case.run(starts, D, H, None, None)
    rows4 = [e * N + 4 for e in range(E)]
    other = [r for r in range(E * N) if r not in rows4]
    for k in ("latent_shift_sq", "state_shift_sq"):
        _plus_zero(zero[k][:, rows4], (k, "of the unseen vehicle"))
        assert bool((zero[k][:, other][:, :, 0, 0] > 0).all()), (k, "a seen vehicle did not move at the first knocked window")
    for q, s in enumerate(starts):
        nw = min(H, J - s)
        assert torch.equal(zero["intent"][:, rows4, q, :nw].cpu(), zero["intent_base"][:, rows4, s:s + nw].cpu()), "the unseen vehicle's intent flipped"
    hold = case.run([2], D, H, None, "hold")                                            # steps 2 .. 4 replaced by the row of step 1
    r7 = 1 * N + 7
    for k in ("latent_shift_sq", "state_shift_sq"):
        _plus_zero(hold[k][:, r7], (k, "of the constant vehicle under hold"))
        assert bool((hold[k][:, r7 - 1, 0, 0] > 0).all())
    _plus_zero(hold["latent_shift_sq"][:, rows4], "hold on the unseen vehicle")
    # invalid windows
    for res, st in ((zero, starts), (hold, [2])):
        for q, s in enumerate(st):
            nw = min(H, J - s)
            for k in JOB_KEYS:
                if nw < H:
                    assert bool((res[k][:, :, q, nw:] == 0).all()), (k, "a window past J is not zero")
    # Z = 1: the softmax is constant
    one = Case(2, 9, 5, 1, 3, 6, 2, device, seed=6)
    got = one.run((0, 3), 2, 4, None, None)
    _plus_zero(got["latent_shift_sq"], "latent_shift_sq with Z = 1")
    assert float(got["state_shift_sq"].max()) > 0.0 and bool((got["intent"] == 0).all())
    return {}


# ------------------------------------------------------------------------------------------------ 4: independence
def check_independence(device):
    """a slot's bits do not depend on its position in ``starts``, on the other jobs or on Q; chains permuted across rows, tiles and envs
    give permuted results; a shorter H gives a prefix; any ``want`` gives the same bits; a contiguous history gives the strided one's;
    repeat calls agree"""
    E, N, d, Z, Lw, J, n_nets = 3, 11, 5, 8, 3, 9, 2
    starts, D, H = (0, 1, 4, 8), 2, 5
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=7)
    full = case.run(starts, D, H, (0, 2), ROW)
    again = case.run(starts, D, H, (0, 2), ROW)
    for k in ALL:
        _same(full[k], again[k], ("repeat", k))
    # subsets and positions (Jn changes with the last start: the base outputs are prefixes)
    for sub in ((1,), (0, 4), (4, 8), (1, 4, 8)):
        part = case.run(sub, D, H, (0, 2), ROW)
        idx = [starts.index(s) for s in sub]
        for k in JOB_KEYS:
            _same(part[k], full[k][:, :, idx], ("subset", sub, k))
        Jn = part["latent"].shape[2]
        _same(part["latent"], full["latent"][:, :, :Jn], ("subset", sub, "latent"))
        _same(part["intent_base"], full["intent_base"][:, :, :Jn], ("subset", sub, "intent_base"))
    # a shorter horizon
    short = case.run(starts, D, 2, (0, 2), ROW)
    for k in JOB_KEYS:
        _same(short[k], full[k][:, :, :, :2], ("shorter H", k))
    # want
    for want in (("latent_shift_sq",), ("intent", "hidden_ko"), ("latent_ko",), ("state_shift_sq", "intent_base")):
        part = case.run(starts, D, H, (0, 2), ROW, want=want)
        for k in set(want) | {"latent"}:
            _same(part[k], full[k], ("want", want, k))
        assert all(part[k] is None for k in ALL if k not in want and k != "latent")
    # contiguous history
    cont = case.run(starts, D, H, (0, 2), ROW, hist=case.hist.to(device))
    for k in ALL:
        _same(cont[k], full[k], ("contiguous history", k))
    # permuted chains: another (env, entity) order, so that chains change row, tile and env
    perm = torch.randperm(E * N, generator=torch.Generator().manual_seed(3))
    flat = case.hist.permute(0, 2, 1, 3, 4).reshape(n_nets, case.T, E * N, d)[:, :, perm]       # [n, T, rows, d]
    hp = flat.reshape(n_nets, case.T, E, N, d).permute(0, 2, 1, 3, 4).contiguous()
    moved = case.run(starts, D, H, (0, 2), ROW, hist=hp.to(device))
    for k in ALL:
        _same(moved[k], full[k][:, perm], ("permuted chains", k))
    return {}


# ------------------------------------------------------------------------------------------------ 5: fp64
def _curr(x, w, Lw):
    zero = torch.zeros_like(x[:, 0])
    return torch.stack([x[:, s] if s >= 0 else zero for s in range(w - Lw + 1, w + 1)], dim=1)


def oracle_chain(p, x, Lw, Jn, dtype):
    """oracle.encoder_forward stepped over windows 0 .. Jn-1 of x [rows, T, d]: (he [rows, Jn, 32], lat [rows, Jn, Z]) in ``dtype``"""
    p = {k: v.to(dtype) for k, v in p.items()}
    x = x.to(dtype)
    rows = x.shape[0]
    h, lat = torch.zeros(rows, 32, dtype=dtype), torch.zeros(rows, p["out.bias"].shape[0], dtype=dtype)
    hs, ls = [], []
    for w in range(Jn):
        _, h, pz = O.encoder_forward(p, _curr(x, w, Lw), h)
        lat = (1.0 - COEF) * lat + pz * COEF
        hs.append(h)
        ls.append(lat)
    return torch.stack(hs, 1), torch.stack(ls, 1)


def _rows(hist_n):
    """[E, T, N, d] -> [rows, T, d]"""
    E, T, N, d = hist_n.shape
    return hist_n.permute(0, 2, 1, 3).reshape(E * N, T, d)


def check_vs_fp64(device, E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline):
    """latent, latent_ko and hidden_ko against the fp64 oracle stepped on the modified history, bound max(1e-5, 1.5 x the fp32 oracle's
    own error); intent and flip where the fp64 chain's top-two margin exceeds that bound (at most 1 % of the entries are left out)"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=11)
    got = case.run(starts, D, H, cols, baseline)
    Jn = min(J, max(starts) + H)
    worst, skipped, total = {}, 0, 0
    Q = len(starts)
    ref = {dt: dict(latent=[], latent_ko=[], hidden_ko=[]) for dt in (torch.float64, torch.float32)}
    for dt in ref:
        for n in range(n_nets):
            _, lat = oracle_chain(case.enc_p[n], _rows(case.hist[n]), Lw, Jn, dt)
            lk, hk = torch.zeros(case.rows, Q, H, Z, dtype=dt), torch.zeros(case.rows, Q, H, 32, dtype=dt)
            for q, s in enumerate(starts):
                nw = min(H, J - s)
                he_c, lat_c = oracle_chain(case.enc_p[n], _rows(case.copy_of(s, D, cols, baseline)[n]), Lw, s + nw, dt)
                lk[:, q, :nw], hk[:, q, :nw] = lat_c[:, s:], he_c[:, s:]
            ref[dt]["latent"].append(lat)
            ref[dt]["latent_ko"].append(lk)
            ref[dt]["hidden_ko"].append(hk)
    r64, r32 = ({k: torch.stack(v) for k, v in ref[dt].items()} for dt in (torch.float64, torch.float32))
    bounds = {}
    for k in ("latent", "latent_ko", "hidden_ko"):
        e32, err = _grad_err(r32[k], r64[k]), _grad_err(got[k], r64[k])
        print("enc_knockout vs fp64", k, "err", err, "e32", e32)
        _worse(worst, k, err)
        _worse(worst, k + "_e32", e32)
        bounds[k] = _bound(e32)
        assert err <= bounds[k], (k, err, e32)
    if Z > 1:
        def sure(lat64, bound):
            top = lat64.topk(2, dim=-1).values
            return (top[..., 0] - top[..., 1]) > bound * float(lat64.abs().max())
        ok_b, ok_k = sure(r64["latent"], bounds["latent"]), sure(r64["latent_ko"], bounds["latent_ko"])
        valid = torch.zeros(Q, H, dtype=torch.bool)
        for q, s in enumerate(starts):
            valid[q, :min(H, J - s)] = True
        ib64, ik64 = r64["latent"].argmax(-1), r64["latent_ko"].argmax(-1)
        assert torch.equal(got["intent_base"].cpu().long()[ok_b], ib64[ok_b])
        m = ok_k & valid
        assert torch.equal(got["intent"].cpu().long()[m], ik64[m])
        win = torch.tensor([[min(s + h, Jn - 1) for h in range(H)] for s in starts])
        both = m & ok_b[:, :, win]
        flip_got = got["intent"].cpu().long() != got["intent_base"].cpu().long()[:, :, win]
        assert torch.equal(flip_got[both], (ik64 != ib64[:, :, win])[both])
        total = int(valid.sum()) * n_nets * case.rows
        skipped = total - int(both.sum())
        print("enc_knockout vs fp64: intent entries inside the margin", skipped, "of", total)
        assert skipped <= MAX_SKIPPED * total, (skipped, total)
        worst["intent_skipped_share"] = skipped / total
    return worst


# ------------------------------------------------------------------------------------------------ 6: sentinels
def check_sentinel(device, E, N, d, Z, Lw, J, n_nets, starts, D, H):
    """outputs and workspace inside sentinel-filled buffers with NaN-poisoned surroundings: exactly the owned slots are written"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=13)
    Q, rows, Jn = len(starts), case.rows, min(J, max(starts) + H)
    shapes = dict(latent=(Jn, Z), intent_base=(Jn,), latent_ko=(Q, H, Z), hidden_ko=(Q, H, 32), intent=(Q, H), latent_shift_sq=(Q, H), state_shift_sq=(Q, H))
    SENT, PAD = 7.0, 64
    big, out = {}, {}
    for k, tail in shapes.items():
        shape = (n_nets, rows) + tail
        n = int(np.prod(shape))
        if k in ("intent_base", "intent"):
            big[k] = torch.full((n + 2 * PAD,), -123456, dtype=torch.int32, device=device)
            big[k][PAD:PAD + n] = 77
        else:
            big[k] = torch.full((n + 2 * PAD,), float("nan"), device=device)
            big[k][PAD:PAD + n] = SENT
        out[k] = big[k][PAD:PAD + n].view(shape)
    wf = n_nets * rows * Jn * 32
    wbig = torch.full((wf + 2 * PAD,), float("nan"), device=device)
    wbig[PAD:PAD + wf] = SENT
    case.run(starts, D, H, None, None, out=out, workspace=wbig[PAD:PAD + wf])
    ref = case.run(starts, D, H, None, None)
    for k in shapes:
        guard = torch.cat([big[k][:PAD], big[k][-PAD:]]).cpu()
        assert bool(torch.isnan(guard).all()) if guard.dtype == torch.float32 else bool((guard == -123456).all()), (k, "wrote outside its tensor")
        mine = out[k].cpu()
        if k in ("latent", "intent_base"):
            _same(mine, ref[k], (k, "in a sentinel buffer"))
            continue
        for q, s in enumerate(starts):
            nw = min(H, J - s)
            _same(mine[:, :, q, :nw], ref[k][:, :, q, :nw], (k, "in a sentinel buffer"))
            rest = mine[:, :, q, nw:]
            assert bool((rest == (77 if mine.dtype == torch.int32 else SENT)).all()), (k, "a slot of a window past J was written")
    wguard = torch.cat([wbig[:PAD], wbig[-PAD:]]).cpu()
    assert bool(torch.isnan(wguard).all()), "wrote outside the workspace"
    assert not bool(torch.isnan(wbig[PAD:PAD + wf]).any())
    return {}


# ------------------------------------------------------------------------------------------------ 7: the method
def summary_numpy(latent_shift, flip, window_valid, hist, starts, D, presence_col):
    """float64 numpy restatement of echo_shift / echo_flip_rate [nA, Q, H]: latent_shift, flip [E, H, nA, Q, N], hist [E, T, nA, N, d];
    sums in environment order, then in vehicle order"""
    E, H, nA, Q, N = latent_shift.shape
    T = hist.shape[1]
    counted = np.zeros((E, H, nA, Q, N), dtype=bool)
    for q, s in enumerate(starts):
        if presence_col is None:
            seen = np.ones((E, nA, N), dtype=bool)
        else:
            seen = (hist[:, s:min(s + D, T), :, :, presence_col] != 0).any(axis=1)      # [E, nA, N]
        counted[:, :, :, q] = seen[:, None] & window_valid[q][None, :, None, None]
    out = []
    for x in (latent_shift.astype(np.float64), flip.astype(np.float64)):
        num, cnt = np.zeros((H, nA, Q, N)), np.zeros((H, nA, Q, N))
        for e in range(E):
            w = counted[e].astype(np.float64)
            num, cnt = num + x[e] * w, cnt + w
        tot, ctot = num[..., 0], cnt[..., 0]
        for i in range(1, N):
            tot, ctot = tot + num[..., i], ctot + cnt[..., i]
        out.append(np.where(ctot > 0, tot / np.maximum(ctot, 1.0), 0.0).transpose(1, 2, 0))
    return out[0], out[1]


def _method_setup(device, tmp_path, E, seed=11, **kw):
    from iplan_amd import synth
    args = BC._e2e_args(device, **kw)
    pol, enc, _ = BC._loaded_policy(args, tmp_path, seed)
    nA, N, d, T = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.episode_limit
    hist = synth.make_history(torch.Generator().manual_seed(5), (E, T, nA), N, d, presence_p=0.7)
    return args, pol, enc, hist


def check_policy_methods(device, tmp_path, E=3):
    """latent_knockout on a loaded checkpoint: every key, shape and dtype; numpy in equals device in; the defaults and H = None;
    latent_ko against latent_trace on the explicit copy and latent against latent_trace; the shifts, flips and the summaries against
    host restatements; the presence_col variants; chunked calls give the unchunked bits with the chunk counts asserted"""
    args, pol, enc, hist = _method_setup(device, tmp_path, E, episode_limit=12)
    nA, N, Lw, T, d, Z = args.n_agents, args.max_vehicle_num, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    J = T - 1 - Lw
    starts, D, H = [0, 3, J - 2], 2, 6
    Q, Jn = len(starts), min(J, J - 2 + H)
    everything = ("shift", "latent_ko", "hidden_ko")
    res = pol.latent_knockout(hist.numpy().astype(np.float64), starts, duration=D, horizon=H, want=everything)
    dev = pol.latent_knockout(hist.to(device), starts, duration=D, horizon=H, want=everything)
    pair = (E, H, nA, Q, N)
    shapes = dict(latent=(E, Jn, nA, N, Z), intent_base=(E, Jn, nA, N), latent_shift=pair, state_shift=pair, intent=pair, flip=pair,
                  latent_ko=pair + (Z,), hidden_ko=pair + (32,), starts=(Q,), window_valid=(Q, H), columns=(d,), echo_shift=(nA, Q, H),
                  echo_flip_rate=(nA, Q, H))
    assert set(res) == set(shapes) | {"window", "direct_windows"} == set(dev), (sorted(res), sorted(dev))
    assert res["window"] == dev["window"] == (D, H) and res["direct_windows"] == dev["direct_windows"] == min(H, D + Lw - 1)
    for k, shape in shapes.items():
        assert isinstance(res[k], np.ndarray) and res[k].shape == shape, (k, res[k].shape, shape)
        assert torch.is_tensor(dev[k]) and dev[k].device.type == torch.device(device).type and tuple(dev[k].shape) == shape, k
        assert np.array_equal(dev[k].cpu().numpy(), res[k]), k
    assert res["flip"].dtype == np.bool_ and res["window_valid"].dtype == np.bool_ and res["latent_shift"].dtype == np.float32
    assert all(res[k].dtype == np.int64 for k in ("intent", "intent_base", "starts", "columns"))
    assert res["echo_shift"].dtype == np.float64 and res["echo_flip_rate"].dtype == np.float64
    assert np.array_equal(res["starts"], starts) and np.array_equal(res["columns"], np.arange(d))
    valid = np.array([[s + h < J for h in range(H)] for s in starts])
    assert np.array_equal(res["window_valid"], valid) and not valid.all()
    # against latent_trace
    trace = pol.latent_trace(hist.numpy())
    assert np.array_equal(res["latent"], trace[:, :Jn])
    h5 = hist.permute(2, 0, 1, 3, 4)                                                    # [nA, E, T, N, d]
    for q, s in enumerate(starts):
        nw = min(H, J - s)
        ref = pol.latent_trace(knocked_copy(h5, s, D, None, None).permute(1, 2, 0, 3, 4).contiguous().numpy())
        assert np.array_equal(res["latent_ko"][:, :nw, :, q], ref[:, s:s + nw]), ("latent_ko vs latent_trace on the copy", q)
        base = res["latent"][:, s:s + nw]
        assert np.array_equal(res["latent_shift"][:, :nw, :, q], _dev_sqrt(host_shift_sq(res["latent_ko"][:, :nw, :, q], base), device))
        assert np.array_equal(res["intent"][:, :nw, :, q], host_argmax(res["latent_ko"][:, :nw, :, q]))
        assert np.array_equal(res["flip"][:, :nw, :, q], res["intent"][:, :nw, :, q] != res["intent_base"][:, s:s + nw])
        for k in ("latent_shift", "state_shift", "intent", "flip", "latent_ko", "hidden_ko"):
            assert not res[k][:, nw:, :, q].any(), (k, "a window past J is not zero")
    assert np.array_equal(res["intent_base"], host_argmax(res["latent"]))
    assert float(res["latent_shift"].max()) > 0.0 and float(res["state_shift"][:, D + Lw - 1:].max()) > 0.0    # ... and an echo
    # an absent vehicle (an all-zero row in the one knocked step the first window reads) is not moved there by the zero baseline
    absent = (hist[:, 3] == 0).all(dim=-1)                                              # [E, nA, N] for the job s = 3
    assert bool(absent.any())
    first = res["state_shift"][:, 0, :, 1]
    assert float(np.abs(first[absent.numpy()]).max()) == 0.0 and float(first[~absent.numpy()].min()) > 0.0
    # the summaries
    for col in (0, 1, None):
        got = pol.latent_knockout(hist.numpy(), starts, duration=D, horizon=H, presence_col=col)
        assert set(got) == set(shapes) - {"latent_ko", "hidden_ko"} | {"window", "direct_windows"}
        assert np.array_equal(got["latent_shift"], res["latent_shift"])
        es, ef = summary_numpy(got["latent_shift"], got["flip"], got["window_valid"], hist.numpy(), starts, D, col)
        assert np.array_equal(got["echo_shift"], es) and np.array_equal(got["echo_flip_rate"], ef), col
        assert (got["echo_shift"][:, valid] > 0).all() and not got["echo_shift"][:, ~valid].any()
    assert not np.array_equal(pol.latent_knockout(hist.numpy(), starts, duration=D, horizon=H, presence_col=None)["echo_shift"], res["echo_shift"])
    gone = hist.clone()
    gone[..., 0] = 0.0                                                                  # nobody is present: nothing counts
    none = pol.latent_knockout(gone.numpy(), starts, duration=D, horizon=H)
    assert float(none["latent_shift"].max()) > 0.0 and not none["echo_shift"].any() and not none["echo_flip_rate"].any()
    # the defaults: D = 1, H = J - min(starts), "shift" only; an int start
    lean = pol.latent_knockout(hist.numpy(), 2)
    assert lean["window"] == (1, J - 2) and lean["latent_shift"].shape == (E, J - 2, nA, 1, N) and lean["window_valid"].all()
    assert "latent_ko" not in lean and lean["latent"].shape == (E, J, nA, N, Z) and np.array_equal(lean["latent"], trace)
    # column subsets and baselines reach the kernel
    feat = pol.latent_knockout(hist.numpy(), starts, duration=D, horizon=H, columns=[1, 2], baseline="hold", want=("latent_ko",))
    ref = pol.latent_trace(knocked_copy(h5, 3, D, [1, 2], "hold").permute(1, 2, 0, 3, 4).contiguous().numpy())
    assert np.array_equal(feat["latent_ko"][:, :J - 3, :, 1], ref[:, 3:]) and np.array_equal(feat["columns"], [1, 2])
    row = np.linspace(-1, 1, nA * d).reshape(nA, d).astype(np.float32)
    by_row = pol.latent_knockout(hist.numpy(), [3], duration=D, horizon=H, baseline=row, want=("latent_ko",))
    ref = pol.latent_trace(knocked_copy(h5, 3, D, None, torch.from_numpy(row)).permute(1, 2, 0, 3, 4).contiguous().numpy())
    assert np.array_equal(by_row["latent_ko"][:, :J - 3, :, 0], ref[:, 3:])
    one_row = pol.latent_knockout(hist.numpy(), [3], duration=D, horizon=H, baseline=row[0], want=("latent_ko",))
    assert np.array_equal(one_row["latent_ko"][:, :, 0], by_row["latent_ko"][:, :, 0])
    # chunks, counted as the method counts them: workspace and base outputs per env, per-job outputs per env and job
    rows1 = nA * N
    base_env = rows1 * Jn * (32 + Z + 1)
    slot = rows1 * H * (3 + Z + 32)
    calls = []
    real = ops.enc_knockout
    ops.enc_knockout = lambda *a, **kw: (calls.append((a[1].shape[1], len(a[2]))), real(*a, **kw))[1]
    try:
        plans = ((E * (base_env + Q * slot), [(E, Q)]), (1.5 * (base_env + Q * slot), [(1, Q)] * E),
                 (base_env + 2.5 * slot, [(1, 2), (1, 1)] * E), (base_env + 1.5 * slot, [(1, 1)] * (Q * E)))
        for floats, plan in plans:
            del calls[:]
            part = pol.latent_knockout(hist.numpy(), starts, duration=D, horizon=H, want=everything, max_workspace_mb=floats * 4 / 2 ** 20)
            assert calls == plan, (floats, calls, plan)
            for k in shapes:
                assert np.array_equal(part[k], res[k]), ("chunked", floats, k)
        try:
            pol.latent_knockout(hist.numpy(), starts, duration=D, horizon=H, want=everything, max_workspace_mb=(base_env + 0.9 * slot) * 4 / 2 ** 20)
            raise AssertionError("a limit below one env and one job was accepted")
        except ValueError:
            pass
    finally:
        ops.enc_knockout = real
    return {"latent_shift_max": float(res["latent_shift"].max()), "echo_state_shift_max": float(res["state_shift"][:, D + Lw - 1:].max())}


def check_config3_widths(device, tmp_path, E=2, N=7):
    """the method at config 3's widths (d = 5, Z = 8, L = 10) against latent_trace on the explicit copy, bit for bit"""
    args, pol, enc, hist = _method_setup(device, tmp_path, E, seed=17, episode_limit=24, max_history_len=10, max_vehicle_num=N, latent_dim=8)
    nA, Lw, T, d, Z = args.n_agents, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    assert (d, Z, Lw) == (5, 8, 10)
    J = T - 1 - Lw
    starts, D, H = [1, 6], 5, 7
    res = pol.latent_knockout(hist.to(device), starts, duration=D, horizon=H, want=("shift", "latent_ko"))
    h5 = hist.permute(2, 0, 1, 3, 4)
    assert torch.equal(res["latent"].cpu(), pol.latent_trace(hist.to(device))[:, :min(J, 6 + H)].cpu())
    for q, s in enumerate(starts):
        ref = pol.latent_trace(knocked_copy(h5, s, D, None, None).permute(1, 2, 0, 3, 4).contiguous().to(device)).cpu()
        assert torch.equal(res["latent_ko"][:, :, :, q].cpu(), ref[:, s:s + H]), q
    assert res["direct_windows"] == H and float(res["echo_shift"].max()) > 0.0
    return {"echo_shift_max": float(res["echo_shift"].max())}


# ------------------------------------------------------------------------------------------------ 8: touches nothing
def check_touches_nothing(device, E=2):
    """parameters, gradients, optimiser state, generators and attributes are unchanged by a call; learn() after latent_knockout() equals
    learn() without it, bit for bit -- also behind a deferred learn, whose decoder update the call joins"""
    args = BC._e2e_args(device)
    f, batch = BC._batch(args, E, device)
    keep = BC._keep(args, E, 21).to(device)
    hist = batch["history"][:, :-1]
    pol = BC._policy(args, 31)
    before = dict(enc=pol.enc_arena.data.clone(), dec=pol.dec_arena.data.clone(), genc=pol.enc_arena.grad.clone(), gdec=pol.dec_arena.grad.clone(),
                  rng=BC._rng_states(device), opt=[str(o.state_dict()) for o in pol.behavior_optimizer], attrs=sorted(vars(pol)), hist=hist.clone())
    pol.latent_knockout(hist, [0, 2], duration=2, horizon=3, want=("shift", "latent_ko", "hidden_ko"), baseline="hold")
    pol.latent_knockout(f["history"][:, :-1].numpy(), 1)
    _sync(device)
    assert torch.equal(pol.enc_arena.data, before["enc"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert torch.equal(pol.enc_arena.grad, before["genc"]) and torch.equal(pol.dec_arena.grad, before["gdec"])
    assert all(torch.equal(x, y) for x, y in zip(BC._rng_states(device), before["rng"]))
    assert [str(o.state_dict()) for o in pol.behavior_optimizer] == before["opt"] and sorted(vars(pol)) == before["attrs"]
    assert torch.equal(hist, before["hist"]), "the history was written"
    results = {}
    for form in ("plain", "with", "deferred", "deferred_with"):
        pol = BC._policy(args, 31)
        if form.startswith("deferred"):
            pol.learn(batch, 0, keep=keep, defer_decoder=True)
        if form.endswith("with"):
            ko = pol.latent_knockout(hist, [1, 3], duration=2, horizon=2)
            assert float(ko["latent_shift"].abs().max()) > 0.0
        losses = pol.learn(batch, 1, keep=keep)
        pol.join_decoder()
        _sync(device)
        results[form] = (np.asarray(losses), pol.enc_arena.data.clone(), pol.dec_arena.data.clone())
    for a, b in (("plain", "with"), ("deferred", "deferred_with")):
        (l0, e0, d0), (l1, e1, d1) = results[a], results[b]
        assert np.array_equal(l0, l1) and torch.equal(e0, e1) and torch.equal(d0, d1), (a, b)
    assert not torch.equal(results["plain"][1], results["deferred"][1])
    return {}


# ------------------------------------------------------------------------------------------------ 9: refusals
def check_kernel_refusals(device):
    """every IPLAN_EINVAL of the entry point, before any launch: the outputs keep their sentinel"""
    case = Case(1, 5, 5, 8, 3, 4, 1, device, seed=9)
    good = case.run((0, 2), 2, 2, None, None)
    a = good["_args"]
    lib = ops._lib(None)
    mark = torch.full_like(good["latent_ko"], 7.0)
    a.latent_ko = mark.data_ptr()

    def refused(text, code="(1)", **fields):
        old = {k: getattr(a, k) for k in fields}
        for k, val in fields.items():
            setattr(a, k, val)
        try:
            lib.call("iplan_enc_knockout", a, L.current_stream(device))
            raise AssertionError(("accepted", fields))
        except L.IplanError as e:
            assert text in str(e), (text, str(e))
        finally:
            for k, val in old.items():
                setattr(a, k, val)

    for bad in (dict(n_nets=0), dict(n_nets=17), dict(E=0), dict(N=0), dict(L=0), dict(L=L.ENC_SAL_MAX_L + 1), dict(T=4), dict(d=0), dict(d=17),
                dict(Z=0), dict(Z=17), dict(Q=0), dict(D=0), dict(H=0)):
        refused("unsupported dims", **bad)
    for ptr in ("hist", "enc_params", "starts", "starts_host", "workspace", "latent"):
        refused("null tensor pointer", **{ptr: None})
    for st, text in (((0, 4), "outside [0, J"), ((-1, 2), "outside [0, J"), ((2, 2), "sorted and distinct"), ((3, 1), "sorted and distinct")):
        host = (C.c_int32 * 2)(*st)
        refused(text, starts_host=C.cast(host, C.c_void_p))
    refused("col_mask", col_mask=0)
    refused("col_mask", col_mask=1 << 5)
    refused("hold=", hold=2)
    refused("exclude each other", hold=1, baseline=good["latent"].data_ptr())
    refused("are needed", workspace_floats=a.workspace_floats - 1)
    refused("16-byte aligned", workspace=a.workspace + 4)
    refused("16-byte aligned", hidden_ko=good["hidden_ko"].data_ptr() + 4)
    assert lib.c.iplan_enc_knockout(None, None) != 0 and b"null args" in lib.c.iplan_last_error()
    _sync(device)
    assert float((mark - 7.0).abs().max()) == 0.0, "a refused call launched"
    lib.call("iplan_enc_knockout", a, L.current_stream(device))                        # the descriptor is whole again
    _sync(device)
    assert torch.equal(mark, good["latent_ko"])
    return {}


def check_method_refusals(device):
    """every ValueError of the method; NotImplementedError from the hard-update and FC policies and for a window longer than the kernel's"""
    args = BC._e2e_args(device)
    pol = BC._policy(args, 41)
    nA, N, Lw, T, d, Z = args.n_agents, args.max_vehicle_num, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    J = T - 1 - Lw
    hist = torch.rand(2, T, nA, N, d)
    ok = pol.latent_knockout(hist.numpy(), [0, J - 1], horizon=2)
    assert ok["latent_shift"].shape == (2, 2, nA, 2, N)
    bad = [dict(history=[[1.0]]), dict(history=hist[0]), dict(history=hist[:, :, :1]), dict(history=hist[..., :d - 1]), dict(history=hist[:, :Lw + 1]),
           dict(starts=[]), dict(starts=[J]), dict(starts=[-1]), dict(starts=[1, 1]), dict(starts=[2, 1]), dict(starts=1.5), dict(starts=[0.0]),
           dict(starts="first"), dict(starts=True), dict(starts=None),
           dict(duration=0), dict(duration=1.0), dict(duration=None), dict(horizon=0), dict(horizon=2.0), dict(horizon="all"),
           dict(columns=[]), dict(columns=[d]), dict(columns=[-1]), dict(columns=[1, 1]), dict(columns=1), dict(columns=[0.5]), dict(columns="all"),
           dict(baseline="zeros"), dict(baseline=np.zeros(d + 1, dtype=np.float32)), dict(baseline=np.zeros((nA + 1, d), dtype=np.float32)),
           dict(baseline=np.zeros(d, dtype=np.int64)), dict(baseline=0.0),
           dict(want=("shifts",)), dict(want="latent"), dict(presence_col=d), dict(presence_col=-1), dict(presence_col=0.5),
           dict(max_workspace_mb=0), dict(max_workspace_mb=-1), dict(max_workspace_mb="1"), dict(max_workspace_mb=1e-6)]
    for kw in bad:
        call = dict(history=hist.numpy() if "history" not in kw else None, starts=[0])
        call.update(kw)
        if torch.is_tensor(call["history"]):
            call["history"] = call["history"].numpy()
        try:
            pol.latent_knockout(**call)
            raise AssertionError(("accepted", kw))
        except ValueError as e:
            assert "latent_knockout" in str(e), (kw, str(e))
    from iplan_amd.nova import behavior_FC_policy, behavior_policy
    for mod, kw in ((behavior_policy, {}), (behavior_FC_policy, dict(behavior_fully_connected=True))):
        other = BC._policy(BC._e2e_args(device, **kw), 41, cls=mod.Behavior_policy)
        try:
            other.latent_knockout(hist.numpy(), [0])
            raise AssertionError("accepted")
        except NotImplementedError as e:
            assert "soft-update" in str(e), str(e)
    long_args = BC._e2e_args(device, max_history_len=L.ENC_SAL_MAX_L + 1, episode_limit=L.ENC_SAL_MAX_L + 4)
    long_pol = BC._policy(long_args, 43)
    try:
        long_pol.latent_knockout(np.zeros((1, L.ENC_SAL_MAX_L + 4, nA, N, d)), [0])
        raise AssertionError("a window longer than the kernel's limit was accepted")
    except NotImplementedError as e:
        assert "max_history_len" in str(e), str(e)
    return {}


# ------------------------------------------------------------------------------------------------ 10: into the policy
def check_policy_continuation(device, E=3):
    """INTEGRATION.md section 1's recipe: latent_ko of job q over windows s .. s+H'-1 is what policy steps s+1 .. s+H' read;
    knockout_trace(entities=[-1], start=s+1, override={"behavior_latent": ...}, override_base={"behavior_latent": latent on the same
    windows}) takes it one job at a time.  An override equal to the base gives kl = dlogp = dvalue = +0.0; a real occlusion moves kl"""
    from iplan_amd import synth
    from tests.policy_trace_checks import make_mac
    args = BC._e2e_args(device, episode_limit=9)
    pol = BC._policy(args, 51)
    mac = make_mac(args, 19)
    f = synth.make_episode_fields(args, E, seed=4, terminated_p=0.1)
    f["avail_actions"].scatter_(-1, f["actions"], 1)
    T1 = f["history"].shape[1]
    batch = synth.DictBatch(f, E, T1).to(device)
    Lw = args.max_history_len
    hist = f["history"][:, :-1].to(device)                                              # the steps learn() sees
    J = hist.shape[1] - 1 - Lw
    starts, D, H = [0, 2], 2, 3
    assert max(starts) + H <= J and max(starts) + 1 + H <= T1
    g = pol.latent_knockout(hist, starts, duration=D, horizon=H, want=("shift", "latent_ko"))
    moved = 0.0
    for q, s in enumerate(starts):
        base = g["latent"][:, s:s + H]                                                  # [E, H, nA, N, Z]
        kw = dict(entities=[-1], start=s + 1, duration=H, horizon=H)
        same = mac.knockout_trace(batch, override={"behavior_latent": base[:, :, :, None]}, override_base={"behavior_latent": base}, **kw)
        for k in ("kl", "dlogp", "dvalue"):
            _plus_zero(same[k], (k, "with an override equal to the base"))
        res = mac.knockout_trace(batch, override={"behavior_latent": g["latent_ko"][:, :, :, q:q + 1]}, override_base={"behavior_latent": base}, **kw)
        _sync(device)
        assert res["kl"].shape == (E, H, args.n_agents, 1) and "behavior_latent" in res["overridden"]
        assert bool(torch.isfinite(res["kl"]).all())
        moved = max(moved, float(res["kl"].abs().max()))
    assert moved > 0.0, "a real occlusion left every action distribution where it was"
    return {"kl_max": moved}
