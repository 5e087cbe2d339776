"""TEST INFRASTRUCTURE: the standalone kernels one at a time against plain fp64 references, on whatever library is active --
the host emulator in the CPU suite (tests/test_emu_wgrad.py, test_emu_mlp3.py, test_emu_ac_backward.py, the optimiser tests),
the gfx950 build in tests/test_gpu_kernels.py.  The learner-level parity checks (tests/oracle_checks.py) see these kernels only
summed into a gradient; here every kernel form is reached directly, at the edges of its launch geometry.

Rule (tests/oracle_checks.py): fp64 ground truth, error = max|got - ref64| / max|ref64| per output tensor (``_grad_err``),
bound 1e-5.  Beside every fp64 reference the same thing is computed in plain fp32 torch and its own error e32 is asserted to be
below 6.7e-6, so the widening term of oracle_checks never applies and the bound is the fixed 1e-5.

The checks never touch ``L.use_library_for_tests``: the caller decides which library is active.  Each returns a dict of the
worst errors it saw (the GPU tests log them)."""
import os

import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from tests.oracle_checks import _grad_err
from tests.test_split_bf16 import split3

TOL = 1e-5
E32_MAX = 6.7e-6


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


# ------------------------------------------------------------------------------------------------ wgrad: launch geometry
# csrc/wgrad.hip: wgrad_geom and the trimming of the wide jobs' row chunks in iplan_wgrad, restated (the tests derive their
# row counts and hot-row positions from it; the kernel is not asked)
WG_MIN_ROWS, WG_MAX_CHUNKS, WG_WIDE_SLOTS, WG_WIDE_ROUNDS_MAX = 64, 128, 1024, 1024


def wgrad_kind(O, K):
    OT, KT = (O + 15) // 16, (K + 15) // 16
    if OT > 8:
        return "wide"
    return "thin_k" if KT <= 1 else ("thin_o" if OT == 1 else "square")


def wgrad_wide_jobs(O, K):
    OT, KT = (O + 15) // 16, (K + 15) // 16
    return ((OT + 11) // 12) * max(1, (KT + 3) // 4) if OT > 8 else 0


def wgrad_chunks_wide(wide_jobs, n_nets):
    if wide_jobs == 0:
        return WG_MAX_CHUNKS
    per_chunk = wide_jobs * n_nets
    rounds = min(WG_WIDE_ROUNDS_MAX, max(1, per_chunk * WG_MAX_CHUNKS // WG_WIDE_SLOTS))
    return max(1, min(WG_MAX_CHUNKS, rounds * WG_WIDE_SLOTS // per_chunk))


def wgrad_chunking(O, K, rows, chunks_wide=WG_MAX_CHUNKS):
    """(target, vrows, vchunks) of a problem"""
    kind = wgrad_kind(O, K)
    target = chunks_wide if kind == "wide" else (8 * WG_MAX_CHUNKS if kind in ("thin_k", "thin_o") else WG_MAX_CHUNKS)
    vr = max((rows + target - 1) // target, WG_MIN_ROWS)
    vr = (vr + 15) // 16 * 16
    return target, vr, max(1, (rows + vr - 1) // vr)


def wgrad_rows_at_chunk_target(O, K, chunks_wide=WG_MAX_CHUNKS, vrows=80):
    """a row count at which the problem's virtual chunks reach their target, every chunk is ``vrows`` > IPLAN_WG_MIN_ROWS rows and
    the last one is ragged (not a multiple of 16, nor of the bf16 kernels' 32)"""
    target = wgrad_chunking(O, K, 1, chunks_wide)[0]
    rows = target * vrows - 5
    assert wgrad_chunking(O, K, rows, chunks_wide) == (target, vrows, target) and (rows - (target - 1) * vrows) % 16 != 0
    return rows


# ------------------------------------------------------------------------------------------------ wgrad: operands and launches
class Operand:
    """A row operand of the contraction.  ``logical`` [n_nets, n_outer, n_inner, W] fp32 on the CPU is what the references read;
    the kernel reads the physical copy on ``device``: row-major, or column-grouped (the behaviour decoder's records
    [tile][16-column group][step][chain][16] with rows = (tile, step * 16 + chain): n_inner = steps * 16, W a multiple of 16)."""

    def __init__(self, logical, device, cg=False):
        self.logical = logical
        n, ro, ri, W = logical.shape
        if cg:
            assert ri % 16 == 0 and W % 16 == 0
            steps, G = ri // 16, W // 16
            phys = logical.reshape(n, ro, steps, 16, G, 16).permute(0, 1, 4, 2, 3, 5).contiguous()
            self.strides, self.cg_stride = (ro * G * steps * 256, G * steps * 256, 16), steps * 256
        else:
            phys = logical.contiguous()
            self.strides, self.cg_stride = (ro * ri * W, ri * W, W), 0
        self.phys = phys.to(device)

    def ptr(self, w0):
        return self.phys.data_ptr() + 4 * w0 * self.strides[2]


def problem(dy, O, x=None, K=0, seg=None, x_col0=0, shift=0, x0=None, w0=0, pre_valid=False, beta=0.0, scale=1.0,
            dw_ld=None, dw_col0=0, want_dw=True, want_db=True):
    """one IplanWgradProblem: dY columns through ``seg`` = (split, c0, c1), X columns from x_col0, rows = the window of inner
    indices [w0, n_inner) of every outer index, X read ``shift`` inner rows away (x0 [n_nets, n_outer, K] / zeros outside the
    window, or in place in front of it with ``pre_valid``)"""
    return dict(dy=dy, O=O, x=x, K=K, seg=seg if seg is not None else (O, 0, 0), x_col0=x_col0, shift=shift, x0=x0, w0=w0,
                pre_valid=pre_valid, beta=beta, scale=scale, dw_ld=K if dw_ld is None else dw_ld, dw_col0=dw_col0,
                want_dw=want_dw and K > 0, want_db=want_db)


def _logical_operands(p, dtype):
    """(dY [n, R, T, O], shifted X [n, R, T, K]) of the window, as the contraction sees them"""
    split, c0, c1 = p["seg"]
    d = p["dy"].logical.to(dtype)
    d = torch.cat([d[..., c0:c0 + split], d[..., c1:c1 + p["O"] - split]], -1)[:, :, p["w0"]:]
    if not p["K"]:
        return d, None
    xf = p["x"].logical.to(dtype)[..., p["x_col0"]:p["x_col0"] + p["K"]]
    T, s, w0 = xf.shape[2], p["shift"], p["w0"]
    src = torch.arange(w0, T) + s                                # the inner index each window row reads
    lo = 0 if (p["pre_valid"] and s < 0) else w0                 # first inner index that may be read in place
    valid = (src >= lo) & (src < T)
    xs = xf[:, :, src.clamp(0, T - 1)] * valid.to(dtype)[None, None, :, None]
    if p["x0"] is not None:
        assert s == -1 and not p["pre_valid"]
        xs[:, :, 0] = p["x0"].to(dtype)
    return d, xs


def _blocked_sum(f, *ops, block=256):
    """sum over all rows of f(row block): the references' contraction in blocks of 256 rows whose partial results are then added,
    in the operands' own dtype.  For fp64 the order is immaterial; for the fp32 reference it fixes a summation that does not
    depend on which path the host's torch takes for a long, thin contraction (its one-call fp32 einsum of the 81 915-row thin-O
    case was 3.6e-7 from fp64 on one host and 7.6e-6 on another -- an error of that reference, not a property of the inputs)"""
    flat = [t.reshape(t.shape[0], -1, t.shape[-1]) for t in ops]
    parts = [f(*[t[:, r0:r0 + block] for t in flat]) for r0 in range(0, flat[0].shape[1], block)]
    return torch.stack(parts).sum(0)


def run_wgrad(device, n_nets, problems):
    """ONE Wgrad.run() of ``problems`` into a fresh arena that is pre-filled with a sentinel pattern.  Asserts that every float
    outside the regions the problems own -- the skipped columns of a dw_ld-strided destination included -- is bit-identical
    to the sentinel afterwards.  Returns (arena on the CPU, per problem dict(dw, db, dw64, db64, dw32, db32)); the
    references include the beta * (pre-filled destination) term."""
    off, places = 5, []
    for p in problems:
        dw_off = db_off = -1
        if p["want_dw"]:
            dw_off, off = off, off + p["O"] * p["dw_ld"] + 7
        if p["want_db"]:
            db_off, off = off, off + p["O"] + 3
        places.append((dw_off, db_off))
    P = off + 11
    idx = torch.arange(n_nets * P, dtype=torch.float32).reshape(n_nets, P)
    sentinel = 0.5 + (idx % 1021) / 1024.0                       # exact in fp32, no two neighbours alike, the size of the results
    grad = sentinel.clone().to(device)                           # (a copy also on the CPU: the references read the sentinel)
    w = ops.Wgrad(grad, n_nets)
    for p, (dw_off, db_off) in zip(problems, places):
        dy, x = p["dy"], p["x"]
        x0 = p["x0"].contiguous().to(device) if p["x0"] is not None else None
        w.add(dy.ptr(p["w0"]), dy.strides, p["O"], dy.logical.shape[1], dy.logical.shape[2] - p["w0"],
              x=x.ptr(p["w0"]) if p["K"] else None, x_strides=x.strides if p["K"] else (0, 0, 0), K=p["K"], dw_off=dw_off, db_off=db_off,
              dw_ld=p["dw_ld"], dw_col0=p["dw_col0"], seg=p["seg"], x_col0=p["x_col0"], x_shift=p["shift"], x0=x0,
              x0_strides=(x0.stride(0), x0.stride(1)) if x0 is not None else (0, 0), beta=p["beta"], scale=p["scale"],
              dy_cg_stride=dy.cg_stride, x_cg_stride=x.cg_stride if p["K"] else 0, x_pre_valid=p["pre_valid"])
        w._keep += [dy.phys, x.phys if p["K"] else None, x0]
    w.run()
    _sync(device)
    got = grad.cpu()
    owned = torch.zeros(n_nets, P, dtype=torch.bool)
    res = []
    for p, (dw_off, db_off) in zip(problems, places):
        O, K, ld, c0 = p["O"], p["K"], p["dw_ld"], p["dw_col0"]
        r = {}
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            d, xs = _logical_operands(p, dtype)
            if p["want_dw"]:
                pre = sentinel[:, dw_off:dw_off + O * ld].view(n_nets, O, ld)[:, :, c0:c0 + K].to(dtype)
                r["dw" + tag] = p["beta"] * pre + p["scale"] * _blocked_sum(lambda a, b: torch.einsum("nro,nrk->nok", a, b), d, xs)
            if p["want_db"]:
                pre = sentinel[:, db_off:db_off + O].to(dtype)
                r["db" + tag] = p["beta"] * pre + p["scale"] * _blocked_sum(lambda a: a.sum(1), d)
        if p["want_dw"]:
            r["dw"] = got[:, dw_off:dw_off + O * ld].view(n_nets, O, ld)[:, :, c0:c0 + K]
            owned[:, dw_off:dw_off + O * ld].view(n_nets, O, ld)[:, :, c0:c0 + K] = True
        if p["want_db"]:
            r["db"] = got[:, db_off:db_off + O]
            owned[:, db_off:db_off + O] = True
        res.append(r)
    stray = (got.view(torch.int32) != sentinel.view(torch.int32)) & ~owned
    assert not stray.any(), ("floats outside the problems' destinations were written", stray.nonzero()[:8].tolist())
    return got, res


def _assert_vs_fp64(res, worst, what):
    for i, r in enumerate(res):
        for k in ("dw", "db"):
            if k not in r:
                continue
            for n in range(r[k].shape[0]):
                e32 = _grad_err(r[k + "32"][n], r[k + "64"][n])
                err = _grad_err(r[k][n], r[k + "64"][n])
                _worse(worst, k, err)
                _worse(worst, k + "_e32", e32)
                assert e32 < E32_MAX, ("fp32 torch's own error widens the bound: change the inputs", what, i, k, n, e32)
                assert err < TOL, (what, "problem", i, k, "net", n, err)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


# the cases both suites run (tests/test_emu_wgrad.py on the emulator, tests/test_gpu_kernels.py on the GPU)
WGRAD_JOB_SHAPES = [
    (5, 64, 37, 3, 0),         # thin along O  (1 x 4 tiles), ragged rows
    (64, 13, 1000, 1, 0),      # thin along K  (4 x 1), many 8x-short chunks
    (192, 64, 300, 5, -1),     # wide (12 x 4), recurrent operand
    (130, 40, 45, 9, 1),       # wide with ragged tiles on both axes, reverse shift
    (100, 70, 333, 1, 0),      # square jobs (7 x 5 tiles -> 2 x 2 jobs)
    (16, 16, 16, 1, 0),        # exactly one tile, one block
    (7, 0, 50, 2, 0),          # bias only
]
# one (O, K) per job kind; `wide_x0` is the wide job that stays on the fp32 kernel
WGRAD_KINDS = {"thin_k": (64, 13), "thin_o": (5, 64), "square": (100, 70), "wide": (160, 40), "wide_x0": (192, 40)}
# total rows around the chunk geometry: one row, around a 16-row block, around the 64-row minimum chunk (= two 32-row blocks)
WGRAD_EDGE_ROWS = (1, 15, 16, 17, 63, 64, 65)


def check_wgrad_shapes(device, O, K, rows, n_inner, shift, n_nets=2, x0=False, options=False):
    """one problem of wgrad.hip against einsum in fp64: dY rows wider than O and X read from column 2 (the extra columns must be
    ignored); ``x0``: with an initial-state operand (a wide job then stays on the fp32 kernel); ``options``: beta = 1 with
    scale != 1 on the pre-filled destination, dw_ld > K with dw_col0 > 0, and the dY columns through a two-segment map"""
    gen = torch.Generator().manual_seed(O * 1000 + K + 7 * rows + n_inner)
    split = O - O // 3 if options else O
    c1 = split + 4 if options else 0
    dy = Operand(_randn(gen, n_nets, rows, n_inner, O + (7 if options else 3)), device)
    x = Operand(_randn(gen, n_nets, rows, n_inner, K + 5), device) if K else None
    kw = dict(beta=1.0, scale=0.5, dw_ld=K + 9, dw_col0=6, seg=(split, 1, c1)) if options else {}
    p = problem(dy, O, x=x, K=K, x_col0=2 if K else 0, shift=shift, x0=_randn(gen, n_nets, rows, K) if x0 else None, **kw)
    _, res = run_wgrad(device, n_nets, [p])
    worst = {}
    _assert_vs_fp64(res, worst, (O, K, rows, n_inner, shift, n_nets, x0, options))
    return worst


def mixed_launch(device, n_nets=5, rows=150, tiles=3, steps=9, s0=2, seed=0):
    """every job kind in ONE launch: thin-K, thin-O, square, bias only, a single wide job and the two weights of a 64-wide GRU
    on column-grouped records (the paired kernel) -- three wide jobs, so with 5 nets the wide jobs' row chunks are trimmed
    (``wgrad_chunks_wide`` = 68 instead of 128) as they are in production.  Returns the problem list."""
    gen = torch.Generator().manual_seed(1000 + seed + rows + steps)
    H = 64
    dyA = Operand(_randn(gen, n_nets, rows, 3, 170), device)
    xA = Operand(_randn(gen, n_nets, rows, 3, 80), device)
    dyB = Operand(_randn(gen, n_nets, tiles, steps * 16, 21 * 16), device, cg=True)     # [.. 80 | dr dz dn_i (192) | dn_h (64)]
    xB = Operand(_randn(gen, n_nets, tiles, steps * 16, 31 * 16), device, cg=True)      # u at 32, h at 352
    ps = [
        problem(dyA, 64, x=xA, K=13, x_col0=2, beta=1.0, scale=0.5),                                     # thin along K
        problem(dyA, 5, x=xA, K=64, seg=(3, 70, 100), shift=-1),                                         # thin along O
        problem(dyA, 100, x=xA, K=70, x_col0=3, seg=(60, 0, 64), dw_ld=75, dw_col0=4, shift=1),          # square
        problem(dyA, 7, seg=(7, 160, 0)),                                                                # bias only
        problem(dyA, 160, x=xA, K=40, x_col0=1, seg=(150, 2, 155), shift=1, dw_ld=48, dw_col0=8, beta=1.0, scale=-2.0),   # wide, single
        problem(dyB, 3 * H, x=xB, K=H, x_col0=32, seg=(3 * H, 80, 0), w0=s0 * 16),                       # GRU W_ih
        problem(dyB, 3 * H, x=xB, K=H, x_col0=352, seg=(2 * H, 80, 80 + 3 * H), shift=-16, w0=s0 * 16, pre_valid=s0 > 0),   # GRU W_hh
    ]
    assert wgrad_chunks_wide(sum(wgrad_wide_jobs(p["O"], p["K"]) for p in ps), 5) == 68
    return ps


# rows / record steps of the mixed launch at which the wide jobs' chunks reach the trimmed target (68 chunks of 80 rows, the last one
# ragged): 1791 * 3 = 5373 rows of the row-major operands, 3 tiles x 112 steps x 16 = 5376 rows of the records
MIXED_LARGE = dict(rows=1791, tiles=3, steps=114, s0=2)


def check_wgrad_mixed_launch(device, n_nets=5, **kw):
    """(a) the mixed launch against fp64; (c) fixed reduction order: three runs into fresh arenas and one with
    IPLAN_WG_NO_PAIR=1 (the pair as two single wide jobs) are bitwise equal.  Three runs, not a hunt: this checks an
    order of summation, not a race."""
    ps = mixed_launch(device, n_nets, **kw)
    if n_nets == 5 and kw.get("rows") == MIXED_LARGE["rows"]:
        cw = 68
        assert wgrad_chunking(160, 40, 1791 * 3, cw) == (68, 80, 68) and wgrad_chunking(192, 64, 3 * 112 * 16, cw) == (68, 80, 68)
    worst = {}
    first, res = run_wgrad(device, n_nets, ps)
    _assert_vs_fp64(res, worst, "mixed launch")
    for _ in range(2):
        assert torch.equal(run_wgrad(device, n_nets, ps)[0], first), "wgrad is not bitwise reproducible"
    assert os.environ.get("IPLAN_WG_NO_PAIR") is None
    os.environ["IPLAN_WG_NO_PAIR"] = "1"
    try:
        unpaired = run_wgrad(device, n_nets, ps)[0]
    finally:
        del os.environ["IPLAN_WG_NO_PAIR"]
    assert torch.equal(unpaired, first), "the paired GRU launch differs from the two single wide jobs"
    return worst


def check_wgrad_column_grouped(device, O, K, s0, n_nets=2, tiles=3, steps=7):
    """column-grouped operands: dY columns through the segment map, X through x_col0, the recurrent operand read 16 rows back --
    in place where the rows in front of the window exist (x_pre_valid), zeros in front of step 0"""
    gen = torch.Generator().manual_seed(O + K + s0)
    dy = Operand(_randn(gen, n_nets, tiles, steps * 16, 14 * 16), device, cg=True)
    x = Operand(_randn(gen, n_nets, tiles, steps * 16, 9 * 16), device, cg=True)
    p = problem(dy, O, x=x, K=K, x_col0=32, seg=(O, 16, 0), shift=-16, w0=s0 * 16, pre_valid=s0 > 0)
    _, res = run_wgrad(device, n_nets, [p])
    worst = {}
    _assert_vs_fp64(res, worst, ("column grouped", O, K, s0))
    return worst


def check_wgrad_gru_pair(device, s0, steps, tiles, n_nets=2):
    """the two wide problems of a 64-wide GRU on column-grouped records as one paired launch: against fp64, and bit-identical to
    the two unpaired jobs (IPLAN_WG_NO_PAIR=1); ragged row tail, a window that starts past step 0, several row chunks"""
    gen = torch.Generator().manual_seed(steps * 10 + s0)
    H = 64
    dy = Operand(_randn(gen, n_nets, tiles, steps * 16, 21 * 16), device, cg=True)
    x = Operand(_randn(gen, n_nets, tiles, steps * 16, 31 * 16), device, cg=True)
    ps = [problem(dy, 3 * H, x=x, K=H, x_col0=32, seg=(3 * H, 80, 0), w0=s0 * 16),
          problem(dy, 3 * H, x=x, K=H, x_col0=352, seg=(2 * H, 80, 80 + 3 * H), shift=-16, w0=s0 * 16, pre_valid=s0 > 0)]
    paired, res = run_wgrad(device, n_nets, ps)
    worst = {}
    _assert_vs_fp64(res, worst, ("gru pair", s0, steps, tiles))
    assert os.environ.get("IPLAN_WG_NO_PAIR") is None
    os.environ["IPLAN_WG_NO_PAIR"] = "1"
    try:
        plain = run_wgrad(device, n_nets, ps)[0]
    finally:
        del os.environ["IPLAN_WG_NO_PAIR"]
    assert torch.equal(paired, plain)
    return worst


# ------------------------------------------------------------------------------------------------ wgrad: one product at a time
SPLIT_BOUND = 2.0 ** -22       # split-bf16 forms: the 2^-25 dropped-term bound of tests/test_split_bf16.py plus room for the handful
                               # of fp32 roundings when six exact piece products are accumulated
FP32_BOUND = 2.0 ** -24        # fp32 MFMA forms: one rounding of the product
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def _full_mantissa(gen, *shape):
    """values with all 24 significand bits in play, spread over six binades, either sign"""
    m = 1.0 + torch.randint(0, 1 << 23, shape, generator=gen).double() / (1 << 23)
    e = torch.randint(-3, 3, shape, generator=gen).double()
    s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    v = (s * m * 2.0 ** e).float()
    assert torch.equal(v.double(), s * m * 2.0 ** e)
    return v


def _assert_draw_is_sensitive(a, b):
    """the condition that keeps the single-product test honest: in the CPU model of the split form, removing any ONE of the six
    piece products gives a maximum elementwise error of at least 8 x the bound (and all six stay within a quarter of it)"""
    ap, bp = [t.double() for t in split3(a)], [t.double() for t in split3(b)]
    exact = a.double()[:, None] * b.double()[None, :]
    for drop in (None,) + SIX:
        six = sum(ap[i][:, None] * bp[j][None, :] for i, j in SIX if (i, j) != drop)
        err = ((six - exact).abs() / exact.abs()).max().item()
        if drop is None:
            assert err < SPLIT_BOUND / 4, err
        else:
            assert err >= 8 * SPLIT_BOUND, ("the drawn values would not notice a dropped piece product: change the draw", drop, err)


SINGLE_FORMS = ("thin_k", "thin_o", "square", "wide_fp32", "wide_bf16", "pair_bf16")


def check_wgrad_single_products(device, form, rows=70, n_inner=3):
    """dY and X are zero except for one row each, so every dW[o][k] is a single product a[o] * b[k] and every db[o] the single
    value a[o].  One net per hot-row position: the first row, the last row of the ragged tail, the last two rows of the first
    virtual chunk and the first two of the next (from the launch geometry restated above), which with n_inner = 3 also puts the
    hot row at a first, a middle and a last inner step.  For every x_shift in (0, -1, +1) the X row is the dY row's flat
    neighbour on that side: inside the same outer index it is the row the shifted read must return (one product); across an
    outer boundary the read must return zero -- or x0 (fp32 wide form) -- and NOT the neighbour.
    db bit-exact; dW within one rounding (fp32 MFMA forms) / 2^-22 (split-bf16 forms) elementwise.  Returns the measured
    elementwise error per form in units of 2^-24."""
    O, K = dict(thin_k=(64, 13), thin_o=(5, 64), square=(100, 70), wide_fp32=(192, 40), wide_bf16=(160, 64), pair_bf16=(192, 64))[form]
    split = form.endswith("bf16")
    R = rows * n_inner
    probe = 2 if form in ("wide_fp32", "pair_bf16") else 1       # wide jobs per launch (below)
    gen = torch.Generator().manual_seed(len(form) * 100 + O)
    worst = {"units_of_2^-24": 0.0}
    # positions first: the number of nets enters the wide jobs' chunk count
    n_nets = 6
    cw = wgrad_chunks_wide(probe * wgrad_wide_jobs(O, K), n_nets)
    _, vrows, vchunks = wgrad_chunking(O, K, R, cw)
    assert vchunks >= 2 and (R - (vchunks - 1) * vrows) % 16 != 0, "need two chunks and a ragged tail"
    hot = [0, R - 1, vrows - 2, vrows - 1, vrows, vrows + 1]
    assert {h % n_inner for h in hot} == set(range(n_inner))
    for shift in (0, -1, 1):
        a, b = _full_mantissa(gen, O + 64), _full_mantissa(gen, K)
        if split:
            _assert_draw_is_sensitive(a[:O], b)
        dy = torch.zeros(n_nets, R, O + 64 + 3)
        xx = torch.zeros(n_nets, R, K + 5)
        x0 = _full_mantissa(gen, n_nets, rows, K) if form == "wide_fp32" else None
        expect = torch.zeros(n_nets, K, dtype=torch.float64)         # the X row each net's hot dY row must meet
        for n, h in enumerate(hot):
            dy[n, h, 1:1 + O + 64] = a
            hx = h + shift
            if 0 <= hx < R:
                xx[n, hx, 2:2 + K] = b
            inner = h % n_inner + shift
            if 0 <= inner < n_inner:
                expect[n] = b.double()
            elif inner < 0 and x0 is not None:
                expect[n] = x0[n, h // n_inner].double()
        dyo = Operand(dy.view(n_nets, rows, n_inner, -1), device)
        xo = Operand(xx.view(n_nets, rows, n_inner, -1), device)
        main = problem(dyo, O, x=xo, K=K, seg=(O, 1, 0), x_col0=2, shift=shift, x0=x0 if shift == -1 else None)
        ps = [main]
        if form == "wide_fp32":
            # a second wide problem with x0 keeps the whole wide launch on the fp32 kernel for shift 0 / +1 too
            ps.append(problem(dyo, O, x=xo, K=K, seg=(O, 1, 0), x_col0=2, shift=-1, x0=x0, want_db=False))
        if form == "pair_bf16":
            # the mate shares [dr dz] = the first 128 columns and takes its last 64 from further right (same values a[192:256])
            ps.append(problem(dyo, O, x=xo, K=K, seg=(128, 1, 1 + 192), x_col0=2, shift=shift))
        _, res = run_wgrad(device, n_nets, ps)
        for pi, r in enumerate(res[:2 if form == "pair_bf16" else 1]):
            av = a[:O] if pi == 0 else torch.cat([a[:128], a[192:256]])
            if "db" in r:
                assert torch.equal(r["db"], av[None].expand(n_nets, O)), (form, shift, "db is not the hot value bit for bit")
            exact = av.double()[None, :, None] * expect[:, None, :]
            err = (r["dw"].double() - exact).abs()
            lim = (SPLIT_BOUND if split else FP32_BOUND) * exact.abs()
            bad = (err > lim).nonzero()
            assert bad.numel() == 0, (form, "shift", shift, "hot row / o / k", [(hot[n], o, k) for n, o, k in bad[:6].tolist()],
                                      (err / exact.abs().clamp_min(1e-30)).max().item() * 2 ** 24, "x 2^-24")
            nz = exact != 0
            if nz.any():
                _worse(worst, "units_of_2^-24", (err[nz] / exact.abs()[nz]).max().item() * 2 ** 24)
    return worst


# ------------------------------------------------------------------------------------------------ mlp3
class Mlp3Net(torch.nn.Module):
    """the three-layer perceptron csrc/mlp3.hip computes (nova/behavior_FC_net.py's stack)"""

    def __init__(self, k0, h, o):
        super().__init__()
        nn = torch.nn
        self.linear_1, self.linear_2, self.out = nn.Linear(k0, h), nn.Linear(h, h), nn.Linear(h, o)

    def forward(self, x, softmax):
        y = self.out(torch.tanh(self.linear_2(torch.tanh(self.linear_1(x)))))
        return torch.softmax(y, -1) if softmax else y


MLP3_SHAPES = [(20, 32, 8, 37, True), (58, 64, 50, 70, False), (64, 64, 64, 16, False), (5, 32, 3, 129, True)]
# a single row, and one row more than the kernels' 64-row block (4 waves x 16 rows)
MLP3_ROW_EDGES = [(20, 32, 8, 1, True), (58, 64, 50, 1, False), (20, 32, 8, 65, True), (58, 64, 50, 65, False)]


def check_mlp3(device, K0, H, O, rows, softmax, n_nets=2):
    """iplan_mlp3_fwd / _bwd (+ the three wgrad problems of ops.mlp3_backward) against fp64 autograd of the same net: forward, dx,
    every parameter gradient with an explicit upstream gradient; and -- identity output -- the L1 form (loss numerator from the
    forward, -sign(target - out) * scale from the backward) accumulated onto the first gradient (beta = 1)"""
    from iplan_amd.arena import ParamArena
    torch.manual_seed(K0 + O + rows)
    nets = [Mlp3Net(K0, H, O) for _ in range(n_nets)]
    refs = {dt: [Mlp3Net(K0, H, O).to(dt) for _ in range(n_nets)] for dt in (torch.float64, torch.float32)}
    for dt in refs:
        for a, b in zip(nets, refs[dt]):
            b.load_state_dict(a.state_dict())
    arena = ParamArena(nets, device)
    x, g_out, target = torch.randn(n_nets, rows, K0), torch.randn(n_nets, rows, O), torch.randn(n_nets, rows, O)
    worst = {}

    def compare(key, got, r64, r32, what):
        e32, err = _grad_err(r32, r64), _grad_err(got, r64)
        _worse(worst, key, err)
        _worse(worst, key + "_e32", e32)
        assert e32 < E32_MAX, ("fp32 torch's own error widens the bound: change the inputs", what, e32)
        assert err < TOL, (what, err)

    fwd = ops.mlp3_forward(arena, "", x.to(device), H, O, softmax=softmax)
    dx = ops.mlp3_backward(arena, "", fwd, g_out=g_out.to(device), want_dx=True)
    _sync(device)
    first = arena.grad.detach().cpu().clone()
    auto = {}
    for n in range(n_nets):
        for dt in refs:
            xr = x[n].to(dt).requires_grad_(True)
            y = refs[dt][n](xr, softmax)
            (y * g_out[n].to(dt)).sum().backward()
            auto[dt] = (y.detach(), xr.grad, {k: p.grad.clone() for k, p in refs[dt][n].named_parameters()})
            refs[dt][n].zero_grad()
        compare("out", fwd["out"][n], auto[torch.float64][0], auto[torch.float32][0], ("out", n))
        compare("dx", dx[n], auto[torch.float64][1], auto[torch.float32][1], ("dx", n))
        for name in auto[torch.float64][2]:
            compare("grad", arena.grad_of(n, name), auto[torch.float64][2][name], auto[torch.float32][2][name], (name, n))
    if softmax:
        return worst
    fwd = ops.mlp3_forward(arena, "", x.to(device), H, O, target=target.to(device))
    ops.mlp3_backward(arena, "", fwd, g_scale=0.25, beta=1.0)
    _sync(device)
    for n in range(n_nets):
        for dt in refs:
            y = refs[dt][n](x[n].to(dt), False)
            l1 = (target[n].to(dt) - y).abs().sum()
            (l1 * 0.25).backward()
            auto[dt] = (l1.detach(), {k: p.grad.clone() for k, p in refs[dt][n].named_parameters()})
            refs[dt][n].zero_grad()
        compare("l1", fwd["l1"][n], auto[torch.float64][0], auto[torch.float32][0], ("l1", n))
        for name in auto[torch.float64][1]:
            k = arena.off(name)
            before = first[n, k:k + auto[torch.float64][1][name].numel()].view(auto[torch.float64][1][name].shape)
            compare("grad_l1", arena.grad_of(n, name), before.double() + auto[torch.float64][1][name],
                    before + auto[torch.float32][1][name], ("L1 accumulated", name, n))
    return worst


# ------------------------------------------------------------------------------------------------ actor / critic backward
def check_ac_backward(device, n_agents=2, max_vehicle_num=4, E=4, T=5):
    """ops.ac_forward (evaluation mode, saved activations) + ops.ac_backward against fp64 autograd of the oracle: log-probs,
    entropies, values, the new GRU states, and every actor / critic parameter gradient at 1e-5 of the tensor's maximum"""
    from iplan_amd import synth
    from iplan_amd.config import default_args
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    from oracle import iplan_oracle as O
    args = default_args("highway", use_cuda=torch.device(device).type == "cuda", max_vehicle_num=max_vehicle_num, n_agents=n_agents,
                        episode_limit=T)
    torch.manual_seed(3)
    nA, N, T1 = n_agents, max_vehicle_num, T + 1
    mac = DcntrlMAC(synth.make_scheme(args), {"agents": nA}, args)
    f = synth.make_episode_fields(args, E, seed=5, terminated_p=0.3)
    fd = {k: v.to(device) for k, v in f.items()}
    rows = E * T
    srcs = []
    for key, w in (("history", 5), ("attention_latent", 32), ("behavior_latent", 8)):
        t = fd[key]                                      # [E, T1, nA, N, w]
        srcs.append((t, w, t.stride(2), t.stride(1)))
    # last action: action of the previous step (training layout: the action of step 0 at t = 0)
    acts = fd["actions"][..., 0]                         # [E, T1, nA]
    last = torch.cat([acts[:, :1], acts[:, :-1]], 1).to(torch.int32).contiguous()
    spec = ops.AcFeatureSpec(N, srcs, n_actions=5, last_action=last, la_strides=(1, nA), n_id=nA, T=T, T_phys=T1)
    ha, hc, avail, actions = fd["rnn_states_actors"], fd["rnn_states_critics"], fd["avail_actions"], fd["actions"]
    out = ops.ac_forward(mac.actor_arena, mac.critic_arena, 2, spec, rows, nA, h_actor=ha, h_critic=hc,
                         h_strides=(ha.stride(2), ha.stride(1)), avail=avail, avail_strides=(avail.stride(2), avail.stride(1)),
                         mode=2, actions_in=actions, act_strides=(actions.stride(2), actions.stride(1)), n_actions=5,
                         ksplit=1, save=True, want_entropy=True, want_h=True)
    gen = torch.Generator().manual_seed(17)
    g_logp, g_v = torch.randn(nA, rows, generator=gen), torch.randn(nA, rows, generator=gen)
    g_ent = -0.01 / rows
    ops.ac_backward(out, mac.actor_arena, mac.critic_arena, g_logp=g_logp.to(device), g_entropy=g_ent, g_values=g_v.to(device))
    _sync(device)
    worst = {}
    rel = lambda a, b: (a.double().cpu() - b.double()).abs().max().item() / max(1.0, b.abs().max().item())   # noqa: E731
    ha, hc, avail, actions = f["rnn_states_actors"], f["rnn_states_critics"], f["avail_actions"], f["actions"]
    for i in range(nA):
        ap = {k: v.detach().cpu().clone().double().requires_grad_(v.requires_grad) for k, v in mac.agents[i].state_dict(keep_vars=True).items()}
        cp = {k: v.detach().cpu().clone().double().requires_grad_(v.requires_grad) for k, v in mac.critics[i].state_dict(keep_vars=True).items()}
        x = O.build_inputs_train(i, f["history"][:, :, i], f["attention_latent"][:, :, i], f["behavior_latent"][:, :, i],
                                 f["actions_onehot"][:, :, i], nA)[:, :-1].reshape(rows, -1).double()
        lp, _ = O.actor_evaluate(ap, x, ha[:, :-1, i].reshape(rows, -1).double(), actions[:, :-1, i].reshape(rows, 1),
                                 avail[:, :-1, i].reshape(rows, -1))
        logits, ha_new = O.actor_logits(ap, x, ha[:, :-1, i].reshape(rows, -1).double(), avail[:, :-1, i].reshape(rows, -1))
        la = torch.log_softmax(logits, -1)
        ent_rows = -(la.exp() * la).sum(-1)
        v, hc_new = O.critic_value(cp, x, hc[:, :-1, i].reshape(rows, -1).double())
        for key, got, ref in (("logp", out["logp"][i], lp[:, 0]), ("entropy", out["entropy"][i], ent_rows), ("values", out["values"][i], v[:, 0]),
                              ("h_actor", out["h_actor"][i], ha_new), ("h_critic", out["h_critic"][i], hc_new)):
            e = rel(got, ref.detach())
            _worse(worst, key, e)
            assert e < 1e-5, (key, i, e)
        ((lp[:, 0] * g_logp[i].double()).sum() + g_ent * ent_rows.sum()).backward()
        (v[:, 0] * g_v[i].double()).sum().backward()
        for name, prm, arena in (("actor", ap, mac.actor_arena), ("critic", cp, mac.critic_arena)):
            for k in prm:
                got = arena.grad_of(i, k).cpu()
                ref = prm[k].grad if prm[k].grad is not None else torch.zeros_like(prm[k])
                err = (got.double() - ref).abs().max().item()
                _worse(worst, name + "_grad", err / max(ref.abs().max().item(), 1e-30) if ref.abs().max().item() > 0 else err)
                assert err <= 1e-5 * ref.abs().max().item() + 1e-12, (name, i, k, err, ref.abs().max().item())
    return worst


def check_module_level_autograd(device):
    """R_Actor.evaluate_actions / R_Critic.forward / GAT_Net.forward called as plain nn.Modules under autograd (the way the
    reference's learner calls them) give the oracle's fp64 gradients; a second backward accumulates (torch semantics)"""
    from iplan_amd.config import default_args
    from iplan_amd.modules.agents.ippo_actor import R_Actor
    from iplan_amd.modules.critics.ippo_critic import R_Critic
    from iplan_amd.nova.GAT_Net import GAT_Net
    from oracle import iplan_oracle as O
    args = default_args("highway", use_cuda=torch.device(device).type == "cuda", max_vehicle_num=3, n_agents=2)
    torch.manual_seed(11)
    F, R = 40, 19
    actor, critic = R_Actor(F, args), R_Critic(F, args)
    x = torch.randn(R, 1, F)
    h = torch.randn(1, R, 64) * 0.1
    act = torch.randint(0, 5, (R, 1, 1))
    avail = torch.ones(R, 1, 5, dtype=torch.int32)
    avail[::3, 0, 2] = 0
    w = torch.randn(R, 1)
    dx, dh, dact, davail, dw = (t.to(device) for t in (x, h, act, avail, w))
    ap = {k: v.detach().cpu().clone().double().requires_grad_(v.requires_grad) for k, v in actor.state_dict(keep_vars=True).items()}
    cp = {k: v.detach().cpu().clone().double().requires_grad_(v.requires_grad) for k, v in critic.state_dict(keep_vars=True).items()}
    logp, ent = actor.evaluate_actions(dx, dh, dact, davail)
    ((logp * dw).sum() - 0.3 * ent).backward()
    v, _ = critic(dx, dh)
    (v.reshape(-1) * dw.reshape(-1)).sum().backward()
    lp, en = O.actor_evaluate(ap, x[:, 0].double(), h[0].double(), act.reshape(R, 1), avail.reshape(R, 5))
    ((lp * w.double()).sum() - 0.3 * en).backward()
    vv, _ = O.critic_value(cp, x[:, 0].double(), h[0].double())
    (vv[:, 0] * w.reshape(-1).double()).sum().backward()
    worst = {}
    for name, mod, prm in (("actor", actor, ap), ("critic", critic, cp)):
        for k, p in mod.named_parameters():
            if prm[k].grad is None:
                continue
            err = (p.grad.double().cpu() - prm[k].grad).abs().max().item()
            _worse(worst, name + "_grad", err / prm[k].grad.abs().max().item())
            assert err <= 1e-5 * prm[k].grad.abs().max().item() + 1e-12, (k, err)
    # second backward accumulates (torch semantics)
    g1 = actor.base.mlp.fc1[0].bias.grad.clone()
    logp, ent = actor.evaluate_actions(dx, dh, dact, davail)
    ((logp * dw).sum() - 0.3 * ent).backward()
    _sync(device)
    assert torch.allclose(actor.base.mlp.fc1[0].bias.grad, 2 * g1, rtol=1e-5, atol=1e-8)
    # GAT module
    N, D, B = 3, 13, 2
    net = GAT_Net(D, args)
    obs, hp = torch.rand(B, N, D), torch.randn(B * N, 32) * 0.1
    noise = O.gumbel_noise_like_reference(B * N * (N - 1))
    gout = torch.randn(B * N, 32)
    gp = {k: v.detach().cpu().clone().double().requires_grad_(True) for k, v in net.state_dict().items()}
    out = net(obs.to(device), hp.to(device), noise=noise.to(device))
    (out * gout.to(device)).sum().backward()
    o64 = O.gat_forward(gp, obs.double(), hp.double(), noise.double())
    (o64 * gout.double()).sum().backward()
    for k, p in net.named_parameters():
        err = (p.grad.double().cpu() - gp[k].grad).abs().max().item()
        _worse(worst, "gat_grad", err / gp[k].grad.abs().max().item())
        assert err <= 1e-5 * gp[k].grad.abs().max().item() + 1e-10, (k, err)
    return worst


# ------------------------------------------------------------------------------------------------ optimiser
def _rel1(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def check_clip_adam(device):
    """FusedAdam / step_all (iplan_grad_sqnorm + iplan_adam_step) over three steps of three nets -- one of them clipped -- against
    oracle.clip_grad_norm / oracle.adam_step, all nets in one launch (steps 1, 2) and one launch per net (step 3); the
    torch.optim.Adam checkpoint layout of state_dict()"""
    from iplan_amd.arena import ParamArena
    from iplan_amd.optim import FusedAdam, step_all
    from oracle import iplan_oracle as O
    torch.manual_seed(0)
    mods = [torch.nn.Linear(7, 5) for _ in range(3)]
    ref_p = [[p.detach().clone() for p in m.parameters()] for m in mods]
    arena = ParamArena(mods, device)
    opts = [FusedAdam([(arena, i)], lr=1e-2, eps=1e-5) for i in range(3)]
    ref_m = [[torch.zeros_like(p) for p in ps] for ps in ref_p]
    ref_v = [[torch.zeros_like(p) for p in ps] for ps in ref_p]
    worst = {}
    for step in (1, 2, 3):
        grads = [[torch.randn_like(p) * (5.0 if i == 1 else 0.1) for p in ps] for i, ps in enumerate(ref_p)]
        for i, m in enumerate(mods):
            for p, gq in zip(m.parameters(), grads[i]):
                p.grad.copy_(gq)
        if step < 3:
            step_all(opts, 1.0)
        else:
            for o in opts:
                o.step(max_norm=1.0)
        _sync(device)
        for i in range(3):
            gl = [x.clone() for x in grads[i]]
            O.clip_grad_norm(gl, 1.0)
            for k in range(len(gl)):
                O.adam_step(ref_p[i][k], gl[k], ref_m[i][k], ref_v[i][k], step, 1e-2, 1e-5)
            for p, r in zip(mods[i].parameters(), ref_p[i]):
                _worse(worst, "param", _rel1(p.detach(), r))
                assert _rel1(p.detach(), r) < 1e-6
    sd = opts[0].state_dict()
    assert set(sd["state"].keys()) == {0, 1} and sd["state"][0]["exp_avg"].shape == (5, 7)
    return worst


def check_adam_weight_decay(device):
    """weight_decay != 0 (torch.optim.Adam's L2 form, applied after the clip) against torch.optim.Adam itself"""
    from iplan_amd.arena import ParamArena
    from iplan_amd.optim import FusedAdam
    torch.manual_seed(0)
    mods = [torch.nn.Linear(6, 4)]
    ref = torch.nn.Linear(6, 4)
    ref.load_state_dict(mods[0].state_dict())
    arena = ParamArena(mods, device)
    opt = FusedAdam([(arena, 0)], lr=1e-2, eps=1e-5, weight_decay=0.05)
    topt = torch.optim.Adam(ref.parameters(), lr=1e-2, eps=1e-5, weight_decay=0.05)
    worst = {}
    for step in range(3):
        grads = [torch.randn_like(p) * 3 for p in ref.parameters()]
        for p, q, gq in zip(mods[0].parameters(), ref.parameters(), grads):
            p.grad.copy_(gq)
            q.grad = gq.clone()
        opt.step(max_norm=1.0)
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        topt.step()
        _sync(device)
        for p, q in zip(mods[0].parameters(), ref.parameters()):
            _worse(worst, "param", _rel1(p.detach(), q.detach()))
            assert _rel1(p.detach(), q.detach()) < 1e-6
    return worst


class _FlatArena:
    """what optim.grad_sqnorm / optim.adam_launch read of a ParamArena, over nets of exactly ``n`` floats ``stride`` apart (a
    ParamArena pads every tensor to four floats; the kernels take any count and any alignment)"""

    def __init__(self, data, stride, n):
        self.data, self.grad = data, torch.zeros_like(data)
        self._adam_moments = (torch.zeros_like(data), torch.zeros_like(data))
        self.net_stride, self.size, self.version = stride, n, 0


ADAM_SIZES = (1, 255, 256, 257, (1 << 20) + 3)


def check_clip_adam_sizes(device, n, n_nets=5, steps=3, max_norm=1.0, lr=1e-2, eps=1e-5):
    """iplan_grad_sqnorm + iplan_adam_step on five nets of ``n`` parameters (the norm's reductions cross the vector, thread, wave
    and block boundaries; nets 3 floats apart of a multiple of four, so both the 16-byte and the scalar path run) with
    gradient norms far below, far above, exactly at and a hair on either side of max_norm, against the oracle's clip + Adam
    run in fp64: parameters after every step and the clipped gradient at 1e-6, the squared norm at 1e-6 relative (fp32
    torch's own sum of the same data asserted within 6.7e-7)"""
    from iplan_amd import optim
    from oracle import iplan_oracle as O
    gen = torch.Generator().manual_seed(n)
    stride = (n + 3) // 4 * 4 + 3
    p0 = torch.zeros(n_nets, stride)
    p0[:, :n] = torch.randn(n_nets, n, generator=gen)
    arena = _FlatArena(p0.flatten().clone().to(device).view(n_nets, stride), stride, n)
    sq = torch.zeros(n_nets, 2, device=device)
    p64, m64, v64 = p0[:, :n].double().clone(), torch.zeros(n_nets, n, dtype=torch.float64), torch.zeros(n_nets, n, dtype=torch.float64)
    norms = (0.1, 5.0, 1.0, 1.0001, 0.9999)
    worst = {}
    for step in range(1, steps + 1):
        g = torch.randn(n_nets, n, generator=gen)
        g = (g.double() * (torch.tensor(norms[:n_nets], dtype=torch.float64) * max_norm / g.double().norm(dim=1))[:, None]).float()
        gpad = torch.full((n_nets, stride), 7.0)                  # the floats between the nets must not enter the norm
        gpad[:, :n] = g
        arena.grad.copy_(gpad)
        optim.grad_sqnorm(arena, (0, n_nets), sq, 1)
        optim.adam_launch(arena, (0, n_nets), [step] * n_nets, lr, (0.9, 0.999), eps, sq, 1, max_norm)
        _sync(device)
        ref_sq = (g.double() ** 2).sum(1)
        e32 = (((g * g).sum(1).double() - ref_sq).abs() / ref_sq).max().item()
        err = ((sq[:, 1].double().cpu() - ref_sq).abs() / ref_sq).max().item()
        _worse(worst, "sqnorm", err)
        _worse(worst, "sqnorm_e32", e32)
        assert e32 < 6.7e-7, ("fp32 torch's own sum is too far from fp64: fewer elements", n, e32)
        assert err < 1e-6, ("squared norm", n, step, err)
        assert torch.equal(sq[:, 0].cpu(), torch.zeros(n_nets)), "the other slot of the norm buffer was written"
        for k in range(n_nets):
            gl = [g[k].double()]
            O.clip_grad_norm(gl, max_norm)
            O.adam_step(p64[k], gl[0], m64[k], v64[k], step, lr, eps)
            _worse(worst, "clipped_grad", _rel1(arena.grad[k, :n], gl[0]))
            assert _rel1(arena.grad[k, :n], gl[0]) < 1e-6, ("clipped gradient", n, step, k)
        _worse(worst, "param", _rel1(arena.data[:, :n], p64))
        assert _rel1(arena.data[:, :n], p64) < 1e-6, ("parameters", n, step, _rel1(arena.data[:, :n], p64))
        assert torch.equal(arena.grad[:, n:].cpu(), gpad[:, n:]) and torch.equal(arena.data[:, n:].cpu(), p0[:, n:]), "floats between the nets were written"
    return worst


# ------------------------------------------------------------------------------------------------ GAT forward + backward kernels
# iplan_gat_fwd (save=True) + iplan_gat_bwd + the Wgrad job list of ops.gat_backward, called directly.  Unlike the wgrad / mlp3 checks
# above, e32 (the fp32 oracle's own error against fp64) is LOGGED beside the kernel's error, not asserted: at tau >= 0.25 the gumbel
# gate is well conditioned and the bound is the flat TOL; the one tau = 0.01 case (``e32_bound=True``) uses the learner checks'
# data-derived rule max(TOL, E32_FACTOR x e32) (tests/oracle_checks.py) and nothing tighter.
GAT_A = 32                                                       # attention_dim == GAT_hidden_dim of the kernels
GAT_MAX_ENTITIES = 64                                            # IPLAN_MAX_ENTITIES (include/iplan_hip.h)
GAT_EDGE_N = (2, 3, 15, 16, 17, 32, 33, 48, 49, 63, 64)          # around every 16-ego tile boundary, the smallest and the largest scene
GAT_WIDTHS = ((1, 0), (13, 0), (5, 1), (16, 16), (64, 64))       # iplan_gat_fwd's argument check: d0 >= 1, d1 >= 0, no upper limit
# (B, N, d0, d1, tau, kwargs): the cases both suites run
GAT_CASES = ([(2, N, 5, 8, 1.0, {}) for N in GAT_EDGE_N]
             + [(2, 17, d0, d1, 1.0, {}) for d0, d1 in GAT_WIDTHS]
             + [(B, N, 5, 8, 1.0, dict(n_nets=5)) for N in (17, 64) for B in (1, 3)]
             + [(2, N, 5, 8, 1.0, dict(strided=True)) for N in (17, 33)]
             + [(2, 17, 5, 8, 0.25, {})]                          # a 1 / tau applied twice or not at all cannot cancel here
             + [(4, 55, 5, 8, 0.01, dict(e32_bound=True))])       # the shipped gate, at a size where thousands of gates average


def gat_case_id(B, N, d0, d1, tau, kw):
    return f"B{B}_N{N}_d{d0}+{d1}_tau{tau:g}" + "".join(f"_{k}{'' if v is True else v}" for k, v in sorted(kw.items()))


class GatCase:
    """``n_nets`` GAT_Nets with their own weights, inputs, gumbel samples and upstream gradient each (inputs as in
    oracle_checks.check_gat_fwd_bwd_vs_oracle); ``strided``: src0, src1, h_prev, out and g_out are env-major tensors handed to the
    launches as .permute(1, 0, 2, 3) views, as the rollout does"""

    def __init__(self, device, B, N, d0, d1, n_nets=2, noise=True, strided=False, seed=0):
        from iplan_amd.arena import ParamArena
        from iplan_amd.config import default_args
        from iplan_amd.nova.GAT_Net import GAT_Net
        self.device, self.B, self.N, self.d0, self.d1, self.n_nets, self.strided = device, B, N, d0, d1, n_nets, strided
        args = default_args("highway", use_cuda=torch.device(device).type == "cuda", max_vehicle_num=N)
        torch.manual_seed(seed + 1000 * N + 10 * (d0 + d1) + n_nets)
        self.nets = [GAT_Net(d0 + d1, args) for _ in range(n_nets)]
        self.params = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in self.nets]
        self.arena = ParamArena(self.nets, device)
        gen = torch.Generator().manual_seed(seed + 1 + 1000 * N + 10 * (d0 + d1) + n_nets)
        self.src0 = torch.rand(n_nets, B, N, d0, generator=gen) * 2 - 1
        self.src1 = torch.rand(n_nets, B, N, d1, generator=gen) * 2 - 1 if d1 > 0 else None
        self.h_prev = torch.randn(n_nets, B, N, GAT_A, generator=gen) * 0.1
        u = torch.rand(n_nets, B, N, N - 1, 2, generator=gen).clamp_min(1e-20)
        self.noise = -torch.log((-torch.log(u)).clamp_min(1e-20)) if noise else torch.zeros(n_nets, B, N, N - 1, 2)
        self.g_out = torch.randn(n_nets, B, N, GAT_A, generator=gen)
        self.d_src0, self.d_src1, self.d_h, self.d_g = (self._dev(t) for t in (self.src0, self.src1, self.h_prev, self.g_out))
        self.d_noise = self.noise.to(device)

    def _dev(self, t):
        if t is None:
            return None
        if self.strided:
            return t.permute(1, 0, 2, 3).contiguous().to(self.device).permute(1, 0, 2, 3)
        return t.to(self.device)

    def new_out(self):
        if self.strided:
            return torch.empty(self.B, self.n_nets, self.N, GAT_A, device=self.device).permute(1, 0, 2, 3)
        return torch.empty(self.n_nets, self.B, self.N, GAT_A, device=self.device)

    def run(self, tau, out=None):
        """forward (save=True) + backward into self.arena.grad; returns (out, saved)"""
        out, saved = ops.gat_forward(self.arena, self.d_src0, self.d_src1, self.d_h, self.d_noise, tau=tau, save=True,
                                     out=self.new_out() if out is None else out)
        ops.gat_backward(self.arena, saved, self.d_g)
        _sync(self.device)
        return out, saved

    def reference(self, n, tau, dtype):
        """net n through the oracle under autograd: (out [B*N, A], internals incl. q k v, {name: gradient})"""
        from oracle import iplan_oracle as O
        from tests.oracle_checks import _req
        B, N = self.B, self.N
        p = _req(self.params[n], dtype)
        obs = self.src0[n] if self.src1 is None else torch.cat([self.src0[n], self.src1[n]], -1)
        out, it = O.gat_forward(p, obs.to(dtype), self.h_prev[n].reshape(B * N, GAT_A).to(dtype), self.noise[n].reshape(-1, 2).to(dtype),
                                tau=tau, return_internals=True)
        (out * self.g_out[n].reshape(B * N, GAT_A).to(dtype)).sum().backward()
        with torch.no_grad():
            h = it["h"]
            v = torch.relu(h @ p["v.weight"].t() + p["v.bias"])
            it = {k: t.detach() for k, t in it.items()}
            it["qkv"] = torch.cat([h @ p["q.weight"].t(), h @ p["k.weight"].t(), v], -1)
        return out.detach(), it, {k: p[k].grad for k in p}


def check_gat_kernels(device, B, N, d0, d1, tau, n_nets=2, noise=True, strided=False, e32_bound=False):
    """ops.gat_forward(save=True) + ops.gat_backward of ``n_nets`` independent nets against oracle.gat_forward under fp64 autograd,
    EVERY net (the last one sits at the arena's end): out and the saved soft / hard / qkv / x / h_enc at TOL x max(1, |ref|), every
    parameter gradient at TOL of the tensor's own maximum (no floor of 1), nothing NaN or Inf.
    ``e32_bound`` (the tau = 0.01 case only): gradients exactly as oracle_checks.check_gat_fwd_bwd_vs_oracle holds them -- error
    relative to max(1, |ref|), bound max(TOL, E32_FACTOR x the fp32 oracle's own worst error) -- and the saved gate and what it
    feeds (hard, x, out) at max(TOL, E32_FACTOR x the fp32 oracle's error on that tensor): d gate / d logit = 100 gate (1 - gate)."""
    from tests.oracle_checks import E32_FACTOR
    case = GatCase(device, B, N, d0, d1, n_nets, noise, strided)
    out, saved = case.run(tau)
    what = gat_case_id(B, N, d0, d1, tau, dict(n_nets=n_nets, strided=strided))
    worst = {}
    assert torch.isfinite(out).all(), (what, "out is not finite")
    for n in range(n_nets):
        o64, it64, g64 = case.reference(n, tau, torch.float64)
        o32, it32, g32 = case.reference(n, tau, torch.float32)
        got = dict(out=out[n].reshape(B * N, GAT_A), soft=saved["soft"][n].view(B, N, N - 1), hard=saved["hard"][n].view(B, N, N - 1),
                   qkv=saved["qkv"][n].view(B, N, 3 * GAT_A), x=saved["x"][n].view(B, N, GAT_A), h=saved["h_enc"][n].view(B, N, GAT_A))
        it64["out"], it32["out"] = o64, o32
        for k, t in got.items():
            err, e32 = _rel1(t, it64[k]), _rel1(it32[k], it64[k])
            print(what, "net", n, k, "err", err, "fp32 oracle", e32)
            _worse(worst, k, err)
            _worse(worst, k + "_fp32_oracle_vs_fp64", e32)
            bound = max(TOL, E32_FACTOR * e32) if (e32_bound and k in ("hard", "x", "out")) else TOL
            assert err <= bound, (what, "net", n, k, err, bound)
        floor = 1.0 if e32_bound else 1e-30
        scale = {k: max(g64[k].abs().max().item(), floor) for k in g64}
        e32 = max((g32[k].double() - g64[k]).abs().max().item() / scale[k] for k in g64)
        _worse(worst, "fp32_oracle_grad_vs_fp64", e32)
        gtol = max(TOL, E32_FACTOR * e32) if e32_bound else TOL
        for k in g64:
            g = case.arena.grad_of(n, k).cpu()
            assert torch.isfinite(g).all(), (what, "net", n, k, "gradient is not finite")
            err = (g.double() - g64[k]).abs().max().item() / scale[k]
            print(what, "net", n, k, "grad err", err, "of max", g64[k].abs().max().item())
            _worse(worst, "grad", err)
            assert err <= gtol, (what, "net", n, k, err, gtol, "fp32 oracle", e32)
    return worst


def _sentinel(n):
    """n floats exact in fp32, no two neighbours alike, the size of the results"""
    return 0.5 + (torch.arange(n, dtype=torch.float32) % 1021) / 1024.0


def _rehome_grads(arenas, device, fill=None, pad=64):
    """the gradient arenas of ``arenas`` back to back inside ONE buffer with ``pad`` guard floats at either end (what
    ParamArena.colocate_grads does for the GAT + prediction-decoder pair), pre-filled with the sentinel pattern or with ``fill``.
    Returns (buffer, its initial content on the CPU, [(start, stop) of each arena's region])."""
    total = sum(a.grad.numel() for a in arenas) + 2 * pad
    init = _sentinel(total) if fill is None else torch.full((total,), fill)
    big = init.clone().to(device)
    spans, o = [], pad
    for a in arenas:
        n = a.grad.numel()
        a.grad = big[o:o + n].view(a.n_nets, a.size)
        spans.append((o, o + n))
        o += n
    return big, init, spans


def _param_slots(arena):
    """bool [n_nets, size]: the floats of the gradient arena that belong to a parameter (the rest pads tensors to 16 bytes)"""
    own = torch.zeros(arena.n_nets, arena.size, dtype=torch.bool)
    for o, n in arena.ranges():
        own[:, o:o + n] = True
    return own


def _bits_equal(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _decoder_arena(device, d, P, n_nets):
    from iplan_amd.arena import ParamArena
    from iplan_amd.nova.prediction_net import Prediction_Decoder
    mods = [Prediction_Decoder(input_size=d, hidden_size=32, output_size=d, num_layers=1, pred_length=P, teacher_forcing_ratio=0, dropout=0.0)
            for _ in range(n_nets)]
    params = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in mods]
    return ParamArena(mods, device), params


def check_gat_ownership_and_repeatability(device, B=1, N=17, n_nets=2, tau=1.0):
    """``out`` and the GAT gradient arena inside larger sentinel-filled buffers (the gradient arena followed by a prediction-decoder
    arena, as the learner colocates them): after forward + backward the guard floats, the decoder's region and the padding between
    the GAT's tensors are bit-unchanged; pre-filled with NaN instead, no NaN is left in ``out`` or in any GAT parameter's gradient
    (gat_backward fills the gradient, it does not accumulate).  Three runs on the same inputs are bit-identical: the backward
    has no atomics -- per-wave partials are reduced in a fixed order (gat_whh_grad_kernel, phase E, wgrad.hip)."""
    case = GatCase(device, B, N, 5, 8, n_nets, seed=3)
    dec_arena, _ = _decoder_arena(device, 5, 3, n_nets)
    pad, n_out = 64, n_nets * B * N * GAT_A
    runs = []
    for fill in (None, float("nan"), None):
        big, init, (gat_span, dec_span) = _rehome_grads([case.arena, dec_arena], device, fill)
        out_init = _sentinel(n_out + 2 * pad) if fill is None else torch.full((n_out + 2 * pad,), fill)
        out_buf = out_init.clone().to(device)
        out, _ = case.run(tau, out=out_buf[pad:pad + n_out].view(n_nets, B, N, GAT_A))
        got, got_out = big.cpu(), out_buf.cpu()
        own = torch.zeros(big.numel(), dtype=torch.bool)
        own[gat_span[0]:gat_span[1]] = _param_slots(case.arena).flatten()
        assert not torch.isnan(got[own]).any(), "a GAT parameter's gradient was left unwritten"
        assert not torch.isnan(got_out[pad:pad + n_out]).any(), "an element of out was left unwritten"
        assert _bits_equal(got[~own], init[~own]), "gat_backward wrote outside the GAT parameters' gradient slots"
        assert _bits_equal(got_out[:pad], out_init[:pad]) and _bits_equal(got_out[pad + n_out:], out_init[pad + n_out:]), "out's guards were written"
        runs.append((got_out[pad:pad + n_out], got[own]))
    for o, g in runs[1:]:
        assert torch.equal(o, runs[0][0]), "out differs between runs on the same inputs"
        assert torch.equal(g, runs[0][1]), "the GAT gradients differ between runs on the same inputs"
    return {}


def _refused(fn, needle):
    try:
        fn()
    except L.IplanError as e:
        assert needle in str(e), (needle, str(e))
        return
    raise AssertionError(("an invalid argument was accepted", needle))


def check_gat_pdec_bad_arguments(device):
    """the entry points' own argument checks, and nothing they do not reject: iplan_gat_fwd refuses N = 1 and N = IPLAN_MAX_ENTITIES
    + 1 (csrc/gat.hip: check_gat, N outside [2, 64]); iplan_pdec_fwd refuses d = 17, d = 0, rows % N != 0 and P = 0 (csrc/preddec.hip:
    check_pdec).  The refusal comes before the launch: the outputs keep their sentinel, and the same descriptor with the field
    restored gives the first run's bits."""
    lib = ops._lib(None)
    stream = L.current_stream(device)
    case = GatCase(device, 1, 3, 5, 8, 1, seed=5)
    good, saved = ops.gat_forward(case.arena, case.d_src0, case.d_src1, case.d_h, case.d_noise, tau=1.0, save=True)
    _sync(device)
    good = good.clone()
    a = saved["_args"]
    sent = _sentinel(good.numel())
    buf = sent.clone().to(device)
    a.out = buf.data_ptr()
    for N in (1, GAT_MAX_ENTITIES + 1):
        a.N = N
        _refused(lambda: lib.call("iplan_gat_fwd", a, stream), "outside [2,")
    _sync(device)
    assert _bits_equal(buf, sent), "a refused iplan_gat_fwd wrote its output"
    a.N = 3
    lib.call("iplan_gat_fwd", a, stream)
    _sync(device)
    assert torch.equal(buf.view_as(good), good)

    pc = PdecCase(device, 3, 5, 5, 5, 2, None, None, "ones")
    fwd = pc.forward()
    _sync(device)
    a = fwd["_args"]
    bufs = {}
    for k in ("pred", "loss"):
        bufs[k] = (_sentinel(fwd[k].numel()), _sentinel(fwd[k].numel()).to(device))
        setattr(a, k, bufs[k][1].data_ptr())
    for field, bad in (("d", 17), ("d", 0), ("N", 4), ("P", 0)):            # (15 rows: N = 4 does not divide them)
        keep = getattr(a, field)
        setattr(a, field, bad)
        _refused(lambda: lib.call("iplan_pdec_fwd", a, stream), "unsupported dims")
        setattr(a, field, keep)
    _sync(device)
    for k, (sent, buf) in bufs.items():
        assert _bits_equal(buf, sent), (k, "a refused iplan_pdec_fwd wrote its output")
    lib.call("iplan_pdec_fwd", a, stream)
    _sync(device)
    for k, (_, buf) in bufs.items():
        assert torch.equal(buf.view_as(fwd[k]), fwd[k]), k
    return {}


# ------------------------------------------------------------------------------------------------ prediction decoder kernels
# iplan_pdec_fwd / iplan_pdec_loss / iplan_pdec_bwd + the Wgrad job list of ops.pdec_backward, called directly.  16 rows per wave, 4
# waves (64 rows) per workgroup, rows = S * N, d <= 16.  No gate on this path: the bound is the flat TOL.
KINK_MARGIN = 1e-4          # min |target - pred| of the draw: the L1 loss is not differentiable at 0 (asserted, never masked out)


def _pdec_geometry():
    from tests.predict_checks import KERNEL_CASES
    # + 64 rows = exactly one workgroup; 65 rows with N = 5, so that row / N crosses sample boundaries inside a tile; d = 1
    return list(KERNEL_CASES) + [(4, 16, 5, 5, 2), (13, 5, 5, 5, 2), (3, 5, 5, 1, 2), (5, 13, 12, 1, 5)]


PDEC_GEOMETRY = _pdec_geometry()
PDEC_OPTION_SHAPES = [(3, 5, 5, 5, 2), (5, 13, 5, 5, 5)]         # 15 rows; 65 rows, ragged, five nets
PDEC_TEACHERS = (None, "ones", "zeros", "mixed")
PDEC_MASKS = ("ones", "random", "zero_net")
# seeds at which a case's draw keeps KINK_MARGIN (found on the CPU from the fp64 reference alone; 0 where not listed)
PDEC_SEEDS = {
    "S3_N5_P12_d16_n5_keep0_teacher-none_mask-ones": 1,
    "S4_N16_P5_d5_n2_keep0_teacher-none_mask-ones": 1,
    "S5_N13_P12_d1_n5_keep0_teacher-none_mask-ones": 2,
    "S5_N13_P5_d5_n5_keep1_teacher-ones_mask-random": 1,
    "S5_N13_P5_d5_n5_keep0_teacher-mixed_mask-ones": 1,
}
# (S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum): the cases both suites run
PDEC_CASES = ([g + (False, None, "ones", False) for g in PDEC_GEOMETRY]
              + [g + (keep, t, "random", False) for g in PDEC_OPTION_SHAPES for keep in (False, True) for t in PDEC_TEACHERS]
              + [g + (False, "mixed", m, False) for g in PDEC_OPTION_SHAPES for m in ("ones", "zero_net")]     # ("random": in the cross above)
              + [(5, 13, 5, 5, 5, True, t, "random", True) for t in (None, "mixed")])


def pdec_case_id(S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum=False):
    return f"S{S}_N{N}_P{P}_d{d}_n{n_nets}_keep{int(bool(keep))}_teacher-{teacher or 'none'}_mask-{mask_kind}" + ("_masksum" if mask_sum else "")


class PdecCase:
    """random decoder parameters and inputs per net; targets continuous and uniform in [-1, 1].  ``keep``: Bernoulli(0.9) flags with
    drop_p = 0.1, or None; ``teacher``: None, "ones", "zeros", or "mixed" -- a pattern that differs per net: net 0 teaches the even
    steps, the last net only the final step (whose flag must change nothing), the nets between a random draw with a 0 and a 1;
    ``mask_kind``: "ones", "random" (0/1, at least one of each) or "zero_net" (random, all zeros for net 0 of several);
    ``mask_sum``: the injected normaliser, 1.7 x the mask's own sum (0.5 for a net whose mask is all zeros)"""

    def __init__(self, device, S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum=False, seed=None):
        self.device, self.S, self.N, self.P, self.d, self.n_nets = device, S, N, P, d, n_nets
        self.id = pdec_case_id(S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum)
        seed = PDEC_SEEDS.get(self.id, 0) if seed is None else seed
        rows = self.rows = S * N
        torch.manual_seed(seed + 1000 * S + 100 * N + 10 * P + d + n_nets)
        self.arena, self.params = _decoder_arena(device, d, P, n_nets)
        gen = torch.Generator().manual_seed(seed + 7 + S + N + P + d)
        self.x0 = torch.rand(n_nets, rows, d, generator=gen) * 2 - 1
        self.h0 = torch.randn(n_nets, rows, 32, generator=gen) * 0.5
        self.target = torch.rand(n_nets, rows, P, d, generator=gen) * 2 - 1
        self.drop_p = 0.1 if keep else 0.0
        self.keep = (torch.rand(n_nets, P, rows, 32, generator=gen) < 0.9).float() if keep else None
        if mask_kind == "ones":
            self.mask = torch.ones(n_nets, S)
        else:
            assert S >= 2
            self.mask = (torch.rand(n_nets, S, generator=gen) < 0.6).float()
            self.mask[:, 0], self.mask[:, 1] = 1.0, 0.0
            if mask_kind == "zero_net":
                assert n_nets > 1
                self.mask[0] = 0.0
        self.teacher = None
        if teacher == "ones":
            self.teacher = torch.ones(n_nets, P, dtype=torch.int32)
        elif teacher == "zeros":
            self.teacher = torch.zeros(n_nets, P, dtype=torch.int32)
        elif teacher == "mixed":
            t = torch.randint(0, 2, (n_nets, P), generator=gen, dtype=torch.int32)
            if P > 1:
                t[:, 0], t[:, 1] = 1, 0
            t[0] = (torch.arange(P) % 2 == 0).to(torch.int32)
            t[-1] = 0
            t[-1, P - 1] = 1
            self.teacher = t
        self.mask_sum = None
        if mask_sum:
            s = self.mask.sum(1)
            self.mask_sum = torch.where(s > 0, 1.7 * s, torch.full_like(s, 0.5))
        dev = lambda t: None if t is None else t.to(device)  # noqa: E731
        self.d_x0, self.d_h0, self.d_target, self.d_mask, self.d_keep, self.d_teacher, self.d_mask_sum = (
            dev(t) for t in (self.x0, self.h0, self.target, self.mask, self.keep, self.teacher, self.mask_sum))

    def forward(self, teacher="own"):
        return ops.pdec_forward(self.arena, self.d_x0, self.d_h0, self.d_target, self.d_mask, self.N, keep=self.d_keep, drop_p=self.drop_p,
                                teacher=self.d_teacher if isinstance(teacher, str) else teacher, mask_sum=self.d_mask_sum)

    def run(self, teacher="own"):
        fwd = self.forward(teacher)
        g_h0 = ops.pdec_backward(self.arena, fwd)
        _sync(self.device)
        return fwd, g_h0

    def reference(self, n, dtype):
        """net n as a plain loop over the oracle's decoder step: (pred [rows, P, d], loss, {name: gradient}, dLoss/dh0)"""
        from oracle import iplan_oracle as O
        from tests.oracle_checks import _req
        S, N, P, d, rows = self.S, self.N, self.P, self.d, self.rows
        p = _req(self.params[n], dtype)
        dp = O.strip_prefix(p, "decoder.")
        h0 = self.h0[n].to(dtype).requires_grad_(True)
        target = self.target[n].to(dtype)
        x, h, preds = self.x0[n].to(dtype).reshape(rows, 1, d), h0, []
        for s in range(P):
            y, h = O.decoder_forward(dp, x, h, None if self.keep is None else self.keep[n, s].to(dtype).reshape(rows, 1, 32), self.drop_p)
            preds.append(y)
            x = target[:, s:s + 1] if (self.teacher is not None and int(self.teacher[n, s]) != 0) else y
        pred = torch.cat(preds, 1)
        mask_over = self.mask[n].to(dtype)[:, None, None, None].expand(S, N, P, d).reshape(rows, P, d)
        if self.mask_sum is None:
            loss = O.masked_l1(target, pred, mask_over, d * P)
        else:
            loss = (torch.abs(target - pred) * mask_over).sum() / (self.mask_sum[n].to(dtype) * (N * P * d) + O.EPS) * (d * P)
        loss.backward()
        return pred.detach(), loss.detach(), {k: p[k].grad for k in p}, h0.grad


def check_pdec_kernels(device, S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum=False, seed=None):
    """ops.pdec_forward + ops.pdec_backward against the fp64 loop (PdecCase.reference), every net: pred and loss at TOL x max(1, |ref|),
    every decoder parameter's gradient and g_h0 = dLoss/dh0 at TOL of the tensor's own maximum; the fp32 loop's own error is logged
    beside each.  A net whose mask is all zeros has loss 0 and gradients that are exactly 0 (and finite); every masked-out sample's
    rows of g_h0 are exactly 0."""
    case = PdecCase(device, S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum, seed)
    fwd, g_h0 = case.run()
    worst = {}
    margin = float("inf")
    for n in range(n_nets):
        pred64, loss64, g64, gh64 = case.reference(n, torch.float64)
        pred32, loss32, g32, gh32 = case.reference(n, torch.float32)
        margin = min(margin, (case.target[n].double() - pred64).abs().min().item())
        assert margin > KINK_MARGIN, (case.id, "the draw puts a target on the L1 kink: change the seed (PDEC_SEEDS)", n, margin)
        for key, got, r64, r32 in (("pred", fwd["pred"][n], pred64, pred32), ("loss", fwd["loss"][n], loss64, loss32)):
            err = _rel1(got, r64)
            _worse(worst, key, err)
            _worse(worst, key + "_e32", _rel1(r32, r64))
            assert torch.isfinite(got).all() and err <= TOL, (case.id, key, "net", n, err)
        live = case.mask[n].sum() > 0
        named = [(k, case.arena.grad_of(n, k), g64[k], g32[k]) for k in g64] + [("g_h0", g_h0[n], gh64, gh32)]
        for k, got, r64, r32 in named:
            got = got.cpu()
            assert torch.isfinite(got).all(), (case.id, k, "net", n, "not finite")
            if not live:
                assert torch.equal(got, torch.zeros_like(got)), (case.id, k, "net", n, "gradient of an all-masked net is not exactly 0")
                continue
            err = _grad_err(got, r64)
            print(case.id, "net", n, k, "err", err, "e32", _grad_err(r32, r64))
            _worse(worst, "g_h0" if k == "g_h0" else "grad", err)
            _worse(worst, ("g_h0" if k == "g_h0" else "grad") + "_e32", _grad_err(r32, r64))
            assert err <= TOL, (case.id, k, "net", n, err)
        if not live:
            assert float(fwd["loss"][n]) == 0.0 and float(loss64) == 0.0, (case.id, "loss of an all-masked net", n)
        dead = (case.mask[n] == 0)[:, None].expand(S, N).reshape(S * N)
        rows_dead = g_h0[n].cpu()[dead]
        assert torch.equal(rows_dead, torch.zeros_like(rows_dead)), (case.id, "a masked-out sample contributes to g_h0", n)
    worst["kink_margin"] = margin
    return worst


def check_pdec_teacher_identities(device):
    """``teacher`` all zeros is bit-identical to teacher=None (pred, loss, gradients, g_h0); so is all ones at P = 1, where the only
    flag is the last step's and feeds nothing"""
    for (S, N, P, d, n_nets), flag in (((5, 13, 5, 5, 5), 0), ((1, 17, 1, 4, 2), 1)):
        results = []
        for teacher in (None, torch.full((n_nets, P), flag, dtype=torch.int32, device=device)):
            case = PdecCase(device, S, N, P, d, n_nets, True, None, "random" if S > 1 else "ones")
            fwd, g_h0 = case.run(teacher)
            results.append((fwd["pred"].cpu(), fwd["loss"].cpu(), case.arena.grad.cpu().clone(), g_h0.cpu()))
        for name, a, b in zip(("pred", "loss", "grad", "g_h0"), *results):
            assert torch.equal(a, b), ((S, N, P, d, n_nets), "teacher flags", flag, name, "differs from teacher=None")
    return {}


def check_pdec_ownership(device, S=1, N=17, P=5, d=5, n_nets=2):
    """17 rows (a ragged second tile), two nets.  The decoder's gradient arena sits behind a GAT arena inside one sentinel-filled
    buffer, as the learner colocates them: pdec_backward leaves the guards, the GAT's region and the padding between the decoder's
    tensors bit-unchanged, and -- the buffer pre-filled with NaN -- leaves no NaN in any decoder parameter's gradient (it fills,
    it does not accumulate).  pred, loss and g_h0 are allocated by the ops themselves: blocks of their sizes are filled with NaN
    and handed back to the allocator first, so that an element the kernels do not write would surface as a NaN (a caching
    allocator returns exactly those blocks; where it does not, this part checks nothing and costs nothing)."""
    from iplan_amd.arena import ParamArena
    from iplan_amd.config import default_args
    from iplan_amd.nova.GAT_Net import GAT_Net
    case = PdecCase(device, S, N, P, d, n_nets, True, "mixed", "ones")
    args = default_args("highway", use_cuda=torch.device(device).type == "cuda", max_vehicle_num=N)
    gat_arena = ParamArena([GAT_Net(13, args) for _ in range(n_nets)], device)
    rows = S * N
    runs = []
    for fill in (None, float("nan")):
        big, init, (gat_span, dec_span) = _rehome_grads([gat_arena, case.arena], device, fill)
        junk = [torch.full((n,), float("nan"), device=device) for n in
                (n_nets * rows * P * d, n_nets * rows * P * L.PDEC_SAVE, n_nets * ((rows + 15) // 16), n_nets, n_nets * rows * P * L.PDEC_DSAVE,
                 n_nets * rows * 32)]
        _sync(device)
        del junk
        fwd, g_h0 = case.run()
        for k, t in (("pred", fwd["pred"]), ("loss", fwd["loss"]), ("g_h0", g_h0)):
            assert torch.isfinite(t).all(), (k, "has elements the kernels did not write")
        got = big.cpu()
        own = torch.zeros(big.numel(), dtype=torch.bool)
        own[dec_span[0]:dec_span[1]] = _param_slots(case.arena).flatten()
        assert not torch.isnan(got[own]).any(), "a decoder parameter's gradient was left unwritten"
        assert _bits_equal(got[~own], init[~own]), "pdec_backward wrote outside the decoder parameters' gradient slots"
        runs.append((fwd["pred"].cpu(), fwd["loss"].cpu(), g_h0.cpu(), got[own]))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "the decoder kernels' results depend on what their buffers held before"
    return {}
