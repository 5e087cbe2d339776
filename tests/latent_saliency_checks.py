"""TEST INFRASTRUCTURE: intent saliency (csrc/enc_saliency.hip, ops.enc_saliency, Behavior_policy.latent_saliency) on whatever library
is active -- the host emulator in tests/test_emu_latent_saliency.py, the gfx950 build in tests/test_gpu_latent_saliency.py.

Reference: the encoder chain of ``latent_trace`` restated window by window from oracle.gru_seq / oracle.encoder_forward's arithmetic
(``_window``; checked against oracle.encoder_forward itself), in torch fp64 and fp32 with autograd.  The history is ONE leaf shared by
the overlapping windows, he of the window in front of the truncation is a second leaf (carry_l2), and the ReLU goes through
oracle._relu_hinted with the branch the kernel took (its ``active`` mask): a gradient is compared on the same branch.
Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor (``_grad_err``),
bound = max(1e-5, E32_FACTOR x the fp32 restatement's own error against fp64 on the same branches).  No other hand-set number.
The checks never touch ``L.use_library_for_tests``: the caller decides which library is active.  Each returns the worst errors it saw."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import behavior_eval_checks as BC
from tests.oracle_checks import E32_FACTOR, _grad_err

TOL = 1e-5
COEF = BC.COEF
HINT_DELTA = 1e-5
FULL = "full"
GRAD_KEYS = ("grad", "step_l1", "step_gxi", "feature_l1", "carry_l2")

# (E, N, d, Z, L, J, n_nets, K, windows, target): rows E * N in {1, 16, 17, 33, 65} -- the 16-row tile's edges and one row past a 4-wave
# workgroup; (d, Z) in {(1, 1), (5, 8), (4, 12), (16, 16), (12, 1)}; L in {1, 2, 10}; J in {1, 4, 13}; n_nets in {1, 2, 5};
# K in {0, 1, L - 1, L, full}; windows with j = 0, a j < L - 1 (zero padding inside the window), a j < K (truncation not reached) and
# J - 1, several per launch; the three target forms.  Every listed value at least once, the large ones (65 rows, L = 10, J = 13,
# 5 nets, full K) never all together.
KERNEL_CASES = [
    (1, 1, 1, 1, 1, 1, 1, 0, (0,), "argmax"),
    (2, 8, 5, 8, 10, 13, 2, FULL, (0, 3, 12), "tensor"),
    (1, 17, 4, 12, 2, 4, 5, 1, (0, 1, 3), "int"),
    (3, 11, 16, 16, 10, 4, 1, 10, (0, 2, 3), "argmax"),
    (5, 13, 12, 1, 2, 13, 2, 2, (0, 1, 5, 12), "tensor"),
    (1, 16, 5, 8, 1, 4, 5, 1, (0, 3), "argmax"),
    (5, 13, 5, 8, 10, 13, 1, 9, (0, 4, 12), "int"),
    (1, 33, 4, 12, 2, 13, 1, 0, (0, 12), "tensor"),
    (1, 17, 16, 16, 10, 13, 5, 1, (0, 5, 12), "argmax"),
    (1, 1, 5, 8, 2, 4, 2, FULL, (1, 3), "int"),
    (3, 11, 5, 8, 1, 13, 5, 0, (0, 12), "tensor"),
    (2, 8, 4, 12, 10, 1, 2, 10, (0,), "argmax"),
]


def _sync(device):
    BC._sync(device)


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def _window(p, cur, h0, hint=None):
    """oracle.encoder_forward with the ReLU's branch hinted: cur [rows, L, d], h0 [rows, 32] -> (he [rows, 32], softmax [rows, Z])"""
    u = O._relu_hinted(cur @ p["linear.weight"].t() + p["linear.bias"], hint, HINT_DELTA)
    _, hL = O.gru_seq(u, h0, p["rnn.weight_ih_l0"], p["rnn.weight_hh_l0"], p["rnn.bias_ih_l0"], p["rnn.bias_hh_l0"])
    return hL, torch.softmax(hL @ p["out.weight"].t() + p["out.bias"], dim=-1)


def _curr(x, w, Lw):
    """window w of x [rows, T, d]: steps w-L+1 .. w, zero where the step is negative (right-aligned, as oracle.behavior_windows)"""
    zero = torch.zeros_like(x[:, 0])
    return torch.stack([x[:, s] if s >= 0 else zero for s in range(w - Lw + 1, w + 1)], dim=1)


def unpack_active(active):
    """[.., K+1, L] masks -> bool [.., K+1, L, 32]"""
    a = torch.as_tensor(active).to(torch.int64).cpu() & 0xFFFFFFFF
    return ((a[..., None] >> torch.arange(32)) & 1).bool()


def reference(params, x, windows, K, Lw, v, hints, dtype):
    """One net.  params: encoder state dict, x [rows, T, d], v [rows, nW, Z] cotangents, hints bool [rows, nW, K+1, L, 32] or None.
    Returns dict of grad [rows, nW, R, d], step_l1, step_gxi [rows, nW, R], feature_l1 [rows, nW, d], carry_l2 [rows, nW],
    latent [rows, nW, Z] in ``dtype``: windows j - Kj .. j differentiated, he and the latent in front of them constants."""
    p = {k: t.to(dtype) for k, t in params.items()}
    x = x.to(dtype)
    rows, T, d = x.shape
    Z, R = p["out.bias"].shape[0], K + Lw
    res = {k: [] for k in GRAD_KEYS + ("latent",)}
    # the constants: he_j and lat_j of every window, as latent_trace walks them
    with torch.no_grad():
        h, lat = torch.zeros(rows, 32, dtype=dtype), torch.zeros(rows, Z, dtype=dtype)
        he, lats = [h], [lat]                                             # entry w: the state / latent ENTERING window w
        for w in range(max(windows) + 1):
            h, pz = _window(p, _curr(x, w, Lw), h)
            lat = (1.0 - COEF) * lat + pz * COEF
            he.append(h)
            lats.append(lat)
    for wi, j in enumerate(windows):
        Kj = min(K, j)
        w0 = j - Kj
        xl = x.clone().requires_grad_(True)
        h0 = he[w0].clone().requires_grad_(True)
        h, lat = h0, lats[w0]
        for w in range(w0, j + 1):
            h, pz = _window(p, _curr(xl, w, Lw), h, None if hints is None else hints[:, wi, j - w])
            lat = (1.0 - COEF) * lat + pz * COEF
        y = (lat * v[:, wi].to(dtype)).sum()
        gx, gh = torch.autograd.grad(y, (xl, h0), allow_unused=True)
        gx = torch.zeros_like(x) if gx is None else gx
        G = torch.zeros(rows, R, d, dtype=dtype)
        for r in range(min(R, j + 1)):
            G[:, r] = gx[:, j - r]
        xs = torch.zeros(rows, R, d, dtype=dtype)
        for r in range(min(R, j + 1)):
            xs[:, r] = x[:, j - r]
        res["grad"].append(G)
        res["step_l1"].append(G.abs().sum(-1))
        res["step_gxi"].append((G * xs).sum(-1))
        res["feature_l1"].append(G.abs().sum(-2))
        res["carry_l2"].append(torch.zeros(rows, dtype=dtype) if w0 == 0 or gh is None else torch.linalg.norm(gh, dim=-1))
        res["latent"].append(lat.detach())
    return {k: torch.stack(t, dim=1) for k, t in res.items()}


def step_valid(windows, K, Lw):
    j = np.asarray(windows)[:, None]
    r = np.arange(K + Lw)[None, :]
    return (r <= j) & (r <= np.minimum(K, j) + Lw - 1)


class Case:
    """random encoders and the strided episode buffer of behavior_eval_checks.Case (env, step and net strides larger than packed)"""

    def __init__(self, E, N, d, Z, Lw, J, n_nets, device, seed=0):
        self.base = BC.Case(E, N, Lw, J, d, Z, n_nets, device, seed=seed)            # (its decoder is only used by check_latent_vs_trace)
        self.E, self.N, self.d, self.Z, self.L, self.J, self.n_nets, self.device = E, N, d, Z, Lw, J, n_nets, device
        self.T, self.rows = self.base.T, E * N
        self.enc_p, self.enc_arena = self.base.enc_p, self.base.enc_arena
        self.gen = torch.Generator().manual_seed(1234 + seed)

    @property
    def d_hist(self):
        return self.base.d_hist

    def x(self, net):
        """[rows, T, d] on the host"""
        return self.base.view(self.base.buf)[net].permute(0, 2, 1, 3).reshape(self.rows, self.T, self.d)

    def seed_tensor(self, nW):
        return torch.rand(self.n_nets, self.rows, nW, self.Z, generator=self.gen) * 2 - 1

    def run(self, windows, K, target="argmax", want=ops.ENC_SAL_OUTPUTS, hist=None, seed=None, out=None):
        """target: "argmax", an int, or "tensor" (``seed`` [n, rows, nW, Z] on the host)"""
        kw = dict(seed_index=-1)
        if target == "tensor":
            kw = dict(seed=seed.to(self.device).contiguous())
            want = tuple(k for k in want if k != "target_index")
        elif target != "argmax":
            kw = dict(seed_index=int(target))
        res = ops.enc_saliency(self.enc_arena, self.d_hist if hist is None else hist, list(windows), K, self.L, self.Z, COEF, want=want, out=out, **kw)
        _sync(self.device)
        return res

    def cotangent(self, out, windows, target, seed):
        """[n, rows, nW, Z] on the host: what the launch differentiated"""
        if target == "tensor":
            return seed
        idx = out["target_index"].cpu().long()
        return torch.nn.functional.one_hot(idx, self.Z).to(torch.float32)

    def references(self, out, windows, K, v):
        hints = unpack_active(out["active"])
        r64 = [reference(self.enc_p[n], self.x(n), windows, K, self.L, v[n], hints[n], torch.float64) for n in range(self.n_nets)]
        r32 = [reference(self.enc_p[n], self.x(n), windows, K, self.L, v[n], hints[n], torch.float32) for n in range(self.n_nets)]
        return r64, r32


def _cmp(got, r64, r32, worst, key, what):
    if float(r64.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, (what, key, "reference is exactly zero")
        return
    e32, err = _grad_err(r32, r64), _grad_err(got, r64)
    print(what, key, "err", err, "e32", e32)
    _worse(worst, key, err)
    _worse(worst, key + "_e32", e32)
    assert err <= _bound(e32), (what, key, err, e32)


def assert_vs_fp64(case, out, refs, worst, what, keys=GRAD_KEYS + ("latent",)):
    r64, r32 = refs
    for n in range(case.n_nets):
        for k in keys:
            _cmp(out[k][n], r64[n][k], r32[n][k], worst, k, (what, "net", n))


def assert_structure(case, out, windows, K):
    """what must hold exactly: entries that do not exist are 0.0, no carry where the truncation is not reached, the argmax"""
    sv = torch.as_tensor(step_valid(windows, K, case.L))
    for k in ("grad", "step_l1", "step_gxi"):
        if out.get(k) is not None:
            t = out[k].cpu()
            dead = t[:, :, ~sv] if k != "grad" else t[:, :, ~sv, :]
            assert float(dead.abs().max()) == 0.0 if dead.numel() else True, (k, "an entry that does not exist is not 0.0")
    for wi, j in enumerate(windows):
        if min(K, j) == j and out.get("carry_l2") is not None:
            assert float(out["carry_l2"][:, :, wi].abs().max()) == 0.0, ("carry", j)
        if out.get("active") is not None and min(K, j) < K:
            assert int(out["active"][:, :, wi, min(K, j) + 1:].abs().max()) == 0, ("active of a window that does not exist", j)


def _argmax_ok(out):
    """lowest index on ties (torch.argmax does not promise which one it returns)"""
    lat = out["latent"].cpu()
    first = (lat == lat.max(dim=-1, keepdim=True).values).float().argmax(dim=-1)          # first True
    return torch.equal(out["target_index"].cpu().long(), first)


# ------------------------------------------------------------------------------------------------ (1) the kernel against fp64
def check_kernel(device, E, N, d, Z, Lw, J, n_nets, K, windows, target):
    case = Case(E, N, d, Z, Lw, J, n_nets, device)
    K = max(windows) if K == FULL else K
    seed = case.seed_tensor(len(windows)) if target == "tensor" else None
    tgt = target if target != "int" else (Z - 1) // 2
    out = case.run(windows, K, tgt, seed=seed)
    nW, R = len(windows), K + Lw
    assert out["grad"].shape == (n_nets, E * N, nW, R, d) and out["step_l1"].shape == (n_nets, E * N, nW, R)
    assert out["feature_l1"].shape == (n_nets, E * N, nW, d) and out["carry_l2"].shape == (n_nets, E * N, nW)
    assert out["latent"].shape == (n_nets, E * N, nW, Z) and out["active"].shape == (n_nets, E * N, nW, K + 1, Lw)
    if target == "int":
        assert int((out["target_index"] != tgt).sum()) == 0
    if target != "tensor":
        assert _argmax_ok(out) or target == "int"
    v = case.cotangent(out, windows, target, seed)
    worst = {}
    assert_vs_fp64(case, out, case.references(out, windows, K, v), worst, (E, N, d, Z, Lw, J, n_nets, K, windows, target))
    assert_structure(case, out, windows, K)
    if Z == 1:
        for k in GRAD_KEYS:
            assert float(out[k].abs().max()) == 0.0, (k, "Z = 1: the softmax is constant")
    return worst


# ------------------------------------------------------------------------------------------------ (2) exact zeros
def check_exact_zeros(device):
    """Z = 1: every gradient and the carry are exactly 0.0; entries step_valid excludes are 0.0; no carry where Kj = j; an all-zero
    cotangent gives all zeros"""
    for d, Lw, J, K, windows in ((12, 3, 6, 2, (0, 1, 5)), (1, 10, 4, 1, (0, 3))):
        case = Case(2, 9, d, 1, Lw, J, 2, device, seed=3)
        for target, seed in (("argmax", None), (0, None), ("tensor", case.seed_tensor(len(windows)))):
            out = case.run(windows, K, target, seed=seed)
            for k in GRAD_KEYS:
                assert float(out[k].abs().max()) == 0.0 and not bool(torch.isnan(out[k]).any()), (k, target)
            assert float(out["latent"].min()) > 0.0 and float(out["latent"].max()) <= 1.0          # 1 - (1 - c)^(j + 1)
    case = Case(1, 17, 5, 8, 3, 7, 2, device, seed=4)
    windows, K = (0, 1, 2, 4, 6), 3
    out = case.run(windows, K, "argmax")
    assert_structure(case, out, windows, K)
    sv = step_valid(windows, K, 3)
    assert not sv.all() and float(out["step_l1"].cpu()[:, :, torch.as_tensor(sv)].min()) > 0.0       # ... and the others are not
    assert float(out["carry_l2"][:, :, 3:].min()) > 0.0 and float(out["carry_l2"][:, :, :3].abs().max()) == 0.0
    zero = case.run(windows, K, "tensor", seed=torch.zeros(2, 17, len(windows), 8))
    for k in GRAD_KEYS:
        assert float(zero[k].abs().max()) == 0.0, k
    assert torch.equal(zero["latent"], out["latent"]) and torch.equal(zero["active"], out["active"])
    return {}


# ------------------------------------------------------------------------------------------------ (3) linearity
def check_linearity(device, E=1, N=17, d=5, Z=8, Lw=3, J=6, n_nets=2, K=2, windows=(0, 2, 5)):
    """the result for a cotangent v equals sum_z v_z x the results of the Z index targets, under the bound of (1) (the fp64 reference
    of v, the fp32 restatement's error for v)"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=5)
    seed = case.seed_tensor(len(windows))
    out = case.run(windows, K, "tensor", seed=seed)
    r64, r32 = case.references(out, windows, K, seed)
    combo = {k: torch.zeros_like(out[k], dtype=torch.float64) for k in ("grad",)}
    for z in range(Z):
        oz = case.run(windows, K, z, want=("grad", "active"))
        assert torch.equal(oz["active"], out["active"])                               # the branch does not depend on the cotangent
        combo["grad"] += oz["grad"].double() * seed[:, :, :, z, None, None].to(device).double()
    worst = {}
    for n in range(n_nets):
        e32 = _grad_err(r32[n]["grad"], r64[n]["grad"])
        err = (combo["grad"][n].cpu() - out["grad"][n].double().cpu()).abs().max().item() / r64[n]["grad"].abs().max().item()
        print("linearity net", n, "err", err, "e32", e32)
        _worse(worst, "linearity", err)
        _worse(worst, "linearity_e32", e32)
        assert err <= _bound(e32), (n, err, e32)
    return worst


# ------------------------------------------------------------------------------------------------ (4) placement and repeatability
def check_placement(device, N=19, d=5, Z=8, Lw=3, J=6, n_nets=2, K=2, windows=(0, 2, 3, 5)):
    """bit for bit: a chain moved to another row / tile / env; windows given one at a time against together; a strided history view
    against a contiguous copy; five repeats"""
    case = Case(2, N, d, Z, Lw, J, n_nets, device, seed=6)
    keys = GRAD_KEYS + ("latent", "target_index", "active")
    ref = case.run(windows, K, "argmax")
    for _ in range(4):                                                               # five launches in all
        again = case.run(windows, K, "argmax")
        for k in keys:
            assert torch.equal(again[k], ref[k]), ("repeat", k)
    contig = case.run(windows, K, "argmax", hist=case.d_hist.contiguous())
    assert case.d_hist.stride(2) != contig["_keep"][0].stride(2)
    for k in keys:
        assert torch.equal(contig[k], ref[k]), ("strided against contiguous", k)
    for wi, j in enumerate(windows):
        one = case.run((j,), K, "argmax")
        for k in keys:
            assert torch.equal(one[k][:, :, 0], ref[k][:, :, wi]), ("one window at a time", j, k)
    # the entities in reverse order and the two envs swapped: chain (e, i) sits at row (1 - e) * N + N - 1 - i -- another lane for
    # every chain, another tile for most
    E = 2
    moved = case.d_hist.flip(dims=(1, 3)).contiguous()
    out = case.run(windows, K, "argmax", hist=moved)
    perm = torch.arange(E * N, device=out["grad"].device).flip(0)
    for k in keys:
        assert torch.equal(out[k][:, perm], ref[k]), ("moved chain", k)
    return {}


# ------------------------------------------------------------------------------------------------ (5) writes only what it owns
def check_sentinel(device, E, N, d, Z, Lw, J, n_nets, K, windows):
    """the outputs inside sentinel-filled buffers: floats in front and behind come back unchanged (the padding lanes of a ragged last
    tile write nothing) and every owned entry is written; NaN in OTHER chains' history rows and in steps after a window changes nothing"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=7)
    ref = case.run(windows, K, "argmax")
    keys = GRAD_KEYS + ("latent", "target_index", "active")
    pad = 64
    runs = []
    for shift in (0.0, 0.25):
        bufs, sent, dest = {}, {}, {}
        for k in keys:
            n = ref[k].numel()
            if ref[k].dtype == torch.float32:
                sent[k] = 2.5 + shift + (torch.arange(n + 2 * pad, dtype=torch.float32) % 1021) / 1024.0
            else:
                sent[k] = (torch.arange(n + 2 * pad, dtype=torch.int32) % 1021) + 100000 + int(shift * 4000)
            bufs[k] = sent[k].clone().to(device)
            dest[k] = bufs[k][pad:pad + n].view(ref[k].shape)
        case.run(windows, K, "argmax", out=dest)
        for k in keys:
            got, n = bufs[k].cpu(), ref[k].numel()
            assert torch.equal(got[:pad].view(torch.int32), sent[k][:pad].view(torch.int32)), (k, "entries in front were written")
            assert torch.equal(got[pad + n:].view(torch.int32), sent[k][pad + n:].view(torch.int32)), (k, "entries behind were written")
            assert torch.equal(got[pad:pad + n].view(ref[k].shape), ref[k].cpu()), k
        runs.append({k: bufs[k][pad:pad + ref[k].numel()].cpu() for k in keys})
    for k in keys:                                                                    # written both times: the sentinels differ everywhere
        assert torch.equal(runs[0][k], runs[1][k]), (k, "an owned entry was left unwritten")
    # NaN everywhere but in chain `keep`: its results do not move; NaN in the steps after window j: window j's results do not move
    keep = min(E * N - 1, 3)
    buf = case.base.buf.clone()
    hv = case.base.view(buf)                                                          # [net, E, T, N, d] view of buf
    poisoned = torch.full_like(hv, float("nan"))
    e, i = keep // N, keep % N
    poisoned[:, e, :, i] = hv[:, e, :, i]
    hv.copy_(poisoned)
    out = case.run(windows, K, "argmax", hist=case.base.view(buf.to(device)))
    for k in keys:
        assert torch.equal(out[k][:, keep], ref[k][:, keep]), ("NaN in other chains", k)
    j = windows[0]
    buf = case.base.buf.clone()
    case.base.view(buf)[:, :, j + 1:] = float("nan")
    first = case.run((j,), K, "argmax", hist=case.base.view(buf.to(device)))
    for k in keys:
        assert torch.equal(first[k][:, :, 0], ref[k][:, :, 0]), ("NaN after the window", k)
    return {}


# ------------------------------------------------------------------------------------------------ (6) latent against latent_trace
def check_latent_vs_trace(device, E=2, N=9, d=5, Z=8, Lw=3, J=7, n_nets=2, windows=(0, 1, 4, 6)):
    """lat_j of the target windows against iplan_beh_eval's latent (d + Z <= 16), both under the fp64 bound; whether they are
    bit-identical is reported, not asserted"""
    case = Case(E, N, d, Z, Lw, J, n_nets, device, seed=8)
    out = case.run(windows, 1, "argmax", want=("latent", "active"))
    p64 = {k: t.double() for k, t in case.enc_p[0].items()}                           # the restatement IS the oracle's arithmetic
    cur, h0 = _curr(case.x(0).double(), 1, Lw), torch.rand(E * N, 32, dtype=torch.float64)
    _, hL, lat = O.encoder_forward(p64, cur, h0)
    mine = _window(p64, cur, h0)
    assert torch.equal(mine[0], hL) and torch.equal(mine[1], lat)
    trace = case.base.run(latent=True, recon=False, sums=False)["latent"]             # [n, rows, J, Z]
    v = torch.zeros(n_nets, E * N, len(windows), Z)
    r64, r32 = case.references(out, windows, 1, v)
    worst = {}
    for n in range(n_nets):
        _cmp(out["latent"][n], r64[n]["latent"], r32[n]["latent"], worst, "latent", ("saliency", n))
        _cmp(trace[n][:, list(windows)], r64[n]["latent"], r32[n]["latent"], worst, "trace", ("latent_trace", n))
    same = torch.equal(out["latent"], trace[:, :, list(windows)])
    print("latent bit-identical to iplan_beh_eval's:", same)
    worst["bit_identical_to_latent_trace"] = float(same)
    return worst


# ------------------------------------------------------------------------------------------------ (7) method level
def _method_reference(args, enc, hist, windows, K, res, dtype):
    """grad [E, W, nA, N, R, d], carry [E, W, nA, N], latent [E, W, nA, N, Z] from ``reference`` for the method's own target and branch"""
    E, T, nA, N, d = hist.shape
    Z, Lw = args.latent_dim, args.max_history_len
    hints = unpack_active(res["active"])                                              # [E, W, nA, N, K+1, L, 32]
    v = torch.nn.functional.one_hot(torch.as_tensor(res["target_index"]).long(), Z).float()
    outs = []
    for i in range(nA):
        x = hist[:, :, i].permute(0, 2, 1, 3).reshape(E * N, T, d)
        sel = lambda t: t[:, :, i].permute(0, 2, 1, *range(3, t.dim() - 1)).reshape((E * N, len(windows)) + tuple(t.shape[4:]))
        outs.append(reference(enc[i], x, windows, K, Lw, sel(v), sel(hints), dtype))
    back = lambda k: torch.stack([o[k].reshape((E, N, len(windows)) + tuple(o[k].shape[2:])) for o in outs], dim=2).transpose(1, 3)
    return {k: back(k) for k in GRAD_KEYS + ("latent",)}


def _lag_l1_numpy(step_l1, valid, hist, windows, presence_col):
    """[nA, R] float64 from step_l1 [E, W, nA, N, R], step_valid [W, R] and the presence column of x_j"""
    E, W, nA, N, R = step_l1.shape
    counted = np.broadcast_to(valid[None, :, None, None, :], step_l1.shape).copy()
    if presence_col is not None:
        here = hist[:, list(windows)][..., presence_col] != 0                        # [E, W, nA, N]
        counted &= here[..., None]
    num = (step_l1.astype(np.float64) * counted).sum(axis=(0, 1, 3))
    cnt = counted.sum(axis=(0, 1, 3))
    return np.where(cnt > 0, num / np.maximum(cnt, 1), 0.0), cnt


def check_policy_methods(device, tmp_path, E=3):
    """latent_saliency on a loaded checkpoint: shapes and axis order of everything it returns, numpy and device forms, against the fp64
    reference; lag_l1 against a numpy restatement (presence column, no presence column, nothing counts); target_index = lowest argmax,
    with a tie built from an all-zero out layer; chunked calls give the bits of unchunked ones"""
    args = BC._e2e_args(device, episode_limit=10)
    pol, enc, _ = BC._loaded_policy(args, tmp_path, 11)
    nA, N, Lw, T, d, Z = args.n_agents, args.max_vehicle_num, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    J = T - 1 - Lw
    f, _ = BC._batch(args, E, device)
    hist = f["history"][:, :-1].float().clone()                                       # [E, T, nA, N, d]
    hist[0, :, 0, 1, 0] = 0.0                                                         # a vehicle that is absent (presence column 0) ...
    hist[:, J - 1, 1, 2, 0] = 0.0                                                     # ... and one absent at the last window only
    windows, K = [0, 1, J - 1], 2
    R, W = K + Lw, 3
    everything = ("step", "grad", "act")
    res = pol.latent_saliency(hist.numpy().astype(np.float64), windows=windows, lags=K, want=everything)
    dev = pol.latent_saliency(hist.to(device), windows=windows, lags=K, want=everything)
    shapes = dict(step_l1=(E, W, nA, N, R), step_gxi=(E, W, nA, N, R), feature_l1=(E, W, nA, N, d), grad=(E, W, nA, N, R, d),
                  latent=(E, W, nA, N, Z), step_valid=(W, R), target_index=(E, W, nA, N), carry_l2=(E, W, nA, N), lag_l1=(nA, R),
                  active=(E, W, nA, N, K + 1, Lw))
    assert set(res) == set(shapes) == set(dev), (sorted(res), sorted(dev))
    for k, shape in shapes.items():
        assert isinstance(res[k], np.ndarray) and res[k].shape == shape, (k, res[k].shape, shape)
        assert torch.is_tensor(dev[k]) and dev[k].device.type == torch.device(device).type and tuple(dev[k].shape) == shape, k
        assert np.array_equal(dev[k].cpu().numpy(), res[k]), k
    assert res["step_valid"].dtype == np.bool_ and res["target_index"].dtype == np.int64 and res["active"].dtype == np.int64
    assert res["lag_l1"].dtype == np.float64 and res["grad"].dtype == np.float32
    assert np.array_equal(res["step_valid"], step_valid(windows, K, Lw))
    # axis order: every tensor against the reference laid out [E, W, nA, N, ..]
    r64 = _method_reference(args, enc, hist, windows, K, res, torch.float64)
    r32 = _method_reference(args, enc, hist, windows, K, res, torch.float32)
    worst = {}
    for k in GRAD_KEYS + ("latent",):
        for i in range(nA):
            _cmp(torch.as_tensor(res[k])[:, :, i], r64[k][:, :, i], r32[k][:, :, i], worst, k, ("agent", i))
    first = (res["latent"] == res["latent"].max(-1, keepdims=True)).argmax(-1)
    assert np.array_equal(res["target_index"], first)
    # the defaults: last window, full lags, "step" only
    lean = pol.latent_saliency(hist.numpy())
    assert set(lean) == {"step_l1", "step_gxi", "feature_l1", "latent", "step_valid", "target_index", "carry_l2", "lag_l1"}
    assert lean["step_l1"].shape == (E, 1, nA, N, J - 1 + Lw) and float(np.abs(lean["carry_l2"]).max()) == 0.0
    one = pol.latent_saliency(hist.numpy(), windows=J - 1, lags=K, want=("grad",))
    assert set(one) == {"grad", "latent", "step_valid", "target_index", "carry_l2", "lag_l1"}
    assert np.array_equal(one["grad"][:, 0], res["grad"][:, 2]) and np.array_equal(one["carry_l2"][:, 0], res["carry_l2"][:, 2])
    # lag_l1
    for col in (0, 1, None):
        got = pol.latent_saliency(hist.numpy(), windows=windows, lags=K, presence_col=col)
        assert np.array_equal(got["step_l1"], res["step_l1"])
        want_l1, cnt = _lag_l1_numpy(got["step_l1"], got["step_valid"], hist.numpy(), windows, col)
        assert np.allclose(got["lag_l1"], want_l1, rtol=1e-12, atol=0.0), (col, got["lag_l1"], want_l1)
        assert (cnt > 0).all() and (got["lag_l1"] > 0).all()
    assert not np.array_equal(pol.latent_saliency(hist.numpy(), windows=windows, lags=K, presence_col=None)["lag_l1"], res["lag_l1"])
    gone = hist.clone()
    gone[..., 0] = 0.0                                                                # nobody is present: nothing counts
    none = pol.latent_saliency(gone.numpy(), windows=windows, lags=K)
    assert float(np.abs(none["step_l1"]).max()) > 0.0 and np.array_equal(none["lag_l1"], np.zeros((nA, R)))
    # int and tensor targets: the tensor form of a one-hot is the int form
    z = 3
    by_int = pol.latent_saliency(hist.numpy(), windows=windows, lags=K, target=z, want=("grad",))
    onehot = np.zeros((E, W, nA, N, Z), dtype=np.float32)
    onehot[..., z] = 1.0
    by_tensor = pol.latent_saliency(hist.numpy(), windows=windows, lags=K, target=onehot, want=("grad",))
    assert "target_index" not in by_int and "target_index" not in by_tensor
    assert np.array_equal(by_int["grad"], by_tensor["grad"]) and float(np.abs(by_int["grad"]).max()) > 0.0
    # chunks, counted as the method counts them (scratch + the chunk's outputs): all envs at once, one env at a time, then one
    # env with two windows / one window at a time -- against the single launch, bit for bit
    rows1 = nA * N
    out_w = rows1 * sum(int(np.prod(shapes[k][4:])) for k in shapes if k not in ("step_valid", "lag_l1"))
    he_env = rows1 * (windows[-1] + 1) * 32
    need1 = he_env + W * (rows1 + out_w)
    calls = []
    real = ops.enc_saliency
    ops.enc_saliency = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        for floats, launches in ((E * need1, 1), (need1 * 1.5, E), (he_env + 2.5 * (rows1 + out_w), 2 * E), (he_env + 1.5 * (rows1 + out_w), 3 * E)):
            del calls[:]
            part = pol.latent_saliency(hist.numpy(), windows=windows, lags=K, want=everything, max_workspace_mb=floats * 4 / 2 ** 20)
            assert len(calls) == launches, (floats, len(calls), launches)
            for k in shapes:
                assert np.array_equal(part[k], res[k]), ("chunked", floats, k)
        try:
            pol.latent_saliency(hist.numpy(), windows=windows, lags=K, want=everything, max_workspace_mb=(he_env + 0.9 * (rows1 + out_w)) * 4 / 2 ** 20)
            raise AssertionError("a limit below one env and one window was accepted")
        except ValueError:
            pass
    finally:
        ops.enc_saliency = real
    # a tie: with an all-zero out layer every latent component is equal, the lowest index wins and the gradient is exactly zero
    for i in range(nA):
        sd = {k: t.clone() for k, t in pol.behavior_encoder[i].state_dict().items()}
        sd["out.weight"].zero_()
        sd["out.bias"].zero_()
        pol.behavior_encoder[i].load_state_dict(sd)
    tie = pol.latent_saliency(hist.numpy(), windows=windows, lags=K, want=("grad",))
    assert np.array_equal(tie["target_index"], np.zeros((E, W, nA, N), dtype=np.int64))
    assert (tie["latent"] == tie["latent"][..., :1]).all() and float(np.abs(tie["grad"]).max()) == 0.0
    return worst


# ------------------------------------------------------------------------------------------------ (8) touches nothing
def check_touches_nothing(device, E=2):
    """parameters, gradients, optimiser state, generators and the carried state are unchanged by a call; learn() after latent_saliency()
    equals learn() without it, bit for bit -- also behind a deferred learn, whose decoder update the call joins"""
    args = BC._e2e_args(device)
    f, batch = BC._batch(args, E, device)
    keep = BC._keep(args, E, 21).to(device)
    hist = batch["history"][:, :-1]
    pol = BC._policy(args, 31)
    before = dict(enc=pol.enc_arena.data.clone(), dec=pol.dec_arena.data.clone(), genc=pol.enc_arena.grad.clone(), gdec=pol.dec_arena.grad.clone(),
                  rng=BC._rng_states(device), opt=[str(o.state_dict()) for o in pol.behavior_optimizer], attrs=sorted(vars(pol)))
    pol.latent_saliency(hist, windows=[0, 2], lags=1, want=("step", "grad", "act"))
    pol.latent_saliency(f["history"][:, :-1].numpy())
    _sync(device)
    assert torch.equal(pol.enc_arena.data, before["enc"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert torch.equal(pol.enc_arena.grad, before["genc"]) and torch.equal(pol.dec_arena.grad, before["gdec"])
    assert all(torch.equal(x, y) for x, y in zip(BC._rng_states(device), before["rng"]))
    assert [str(o.state_dict()) for o in pol.behavior_optimizer] == before["opt"] and sorted(vars(pol)) == before["attrs"]
    results = {}
    for form in ("plain", "with", "deferred", "deferred_with"):
        pol = BC._policy(args, 31)
        if form.startswith("deferred"):
            pol.learn(batch, 0, keep=keep, defer_decoder=True)
        if form.endswith("with"):
            sal = pol.latent_saliency(hist, windows=[1, 3], lags=2, want=("step", "grad"))
            assert float(sal["grad"].abs().max()) > 0.0
        losses = pol.learn(batch, 1, keep=keep)
        pol.join_decoder()
        _sync(device)
        results[form] = (np.asarray(losses), pol.enc_arena.data.clone(), pol.dec_arena.data.clone())
    for a, b in (("plain", "with"), ("deferred", "deferred_with")):
        (l0, e0, d0), (l1, e1, d1) = results[a], results[b]
        assert np.array_equal(l0, l1) and torch.equal(e0, e1) and torch.equal(d0, d1), (a, b)
    assert not torch.equal(results["plain"][1], results["deferred"][1])                # (the second learn really differs from the first)
    # after a deferred learn the call sees the updated encoder: the bits of the same call after an explicit join
    outs = []
    for join in (False, True):
        pol = BC._policy(args, 31)
        pol.learn(batch, 0, keep=keep, defer_decoder=True)
        if join:
            pol.join_decoder()
            _sync(device)
        outs.append(pol.latent_saliency(hist, windows=[1, 3], lags=2, want=("grad",))["grad"].clone())
        pol.join_decoder()
    assert torch.equal(outs[0], outs[1])
    return {}


# ------------------------------------------------------------------------------------------------ (9) refusals
def check_kernel_refusals(device):
    """every IPLAN_EINVAL of the entry point, before any launch: the outputs keep their sentinel"""
    case = Case(1, 5, 5, 8, 3, 4, 1, device, seed=9)
    good = case.run((0, 3), 1, "argmax")
    a = good["_args"]
    lib = ops._lib(None)
    mark = torch.full_like(good["grad"], 7.0)
    a.grad = mark.data_ptr()

    def refused(text, **fields):
        old = {k: getattr(a, k) for k in fields}
        for k, val in fields.items():
            setattr(a, k, val)
        try:
            lib.call("iplan_enc_saliency", a, L.current_stream(device))
            raise AssertionError(("accepted", fields))
        except L.IplanError as e:
            assert text in str(e), (text, str(e))
        finally:
            for k, val in old.items():
                setattr(a, k, val)

    for bad in (dict(n_nets=0), dict(n_nets=17), dict(E=0), dict(N=0), dict(L=0), dict(L=L.ENC_SAL_MAX_L + 1), dict(T=4), dict(d=0), dict(d=17),
                dict(Z=0), dict(Z=17), dict(K=-1), dict(nW=0)):
        refused("unsupported dims", **bad)
    for ptr in ("hist", "enc_params", "windows", "windows_host", "scratch"):
        refused("null tensor pointer", **{ptr: None})
    import ctypes as C
    for wins, text in (((0, 4), "outside [0, J"), ((-1, 2), "outside [0, J"), ((2, 2), "sorted and distinct"), ((3, 1), "sorted and distinct")):
        host = (C.c_int32 * 2)(*wins)
        refused(text, windows_host=C.cast(host, C.c_void_p))
    refused("seed_index", seed_index=8)
    refused("seed_index", seed_index=-2)
    refused("target_index is only defined", seed=good["latent"].data_ptr())
    refused("no output asked for", **{k: None for k in ops.ENC_SAL_OUTPUTS})
    refused("are needed", scratch_floats=a.scratch_floats - 1)
    refused("16-byte aligned", scratch=a.scratch + 4)
    try:
        lib.c.iplan_enc_saliency(None, None)
    except Exception as e:                                                            # (ctypes refuses nothing here: the call returns a code)
        raise AssertionError(e)
    assert lib.c.iplan_enc_saliency(None, None) != 0 and b"null args" in lib.c.iplan_last_error()
    _sync(device)
    assert float((mark - 7.0).abs().max()) == 0.0, "a refused call launched"
    lib.call("iplan_enc_saliency", a, L.current_stream(device))                        # the descriptor is whole again
    _sync(device)
    assert torch.equal(mark, good["grad"])
    return {}


def check_method_refusals(device):
    """every ValueError of the method; NotImplementedError from the hard-update and FC policies and for a window longer than the kernel's"""
    args = BC._e2e_args(device)
    pol = BC._policy(args, 41)
    nA, N, Lw, T, d, Z = args.n_agents, args.max_vehicle_num, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    J = T - 1 - Lw
    hist = torch.rand(2, T, nA, N, d)
    ok = pol.latent_saliency(hist.numpy(), windows=[0, J - 1], lags=0)
    assert ok["step_l1"].shape == (2, 2, nA, N, Lw)
    bad = [dict(history=[[1.0]]), dict(history=hist[0]), dict(history=hist[:, :, :1]), dict(history=hist[..., :d - 1]), dict(history=hist[:, :Lw + 1]),
           dict(windows=[]), dict(windows=[J]), dict(windows=[-1]), dict(windows=[1, 1]), dict(windows=[2, 1]), dict(windows=1.5), dict(windows=[0.0]),
           dict(windows="last"), dict(windows=True),
           dict(lags=-1), dict(lags=1.0), dict(lags="full"),
           dict(target="max"), dict(target=Z), dict(target=-1), dict(target=1.0), dict(target=torch.zeros(2, 1, nA, N, Z + 1)),
           dict(target=torch.zeros(2, 2, nA, N, Z)), dict(target=torch.zeros(2, 1, nA, N, Z, dtype=torch.int64)), dict(target=None),
           dict(want=("steps",)), dict(want="gradient"), dict(presence_col=d), dict(presence_col=-1), dict(presence_col=0.5),
           dict(max_workspace_mb=0), dict(max_workspace_mb=-1), dict(max_workspace_mb="1"), dict(max_workspace_mb=1e-6)]
    for kw in bad:
        call = dict(history=hist.numpy() if "history" not in kw else None)
        call.update(kw)
        if torch.is_tensor(call["history"]):
            call["history"] = call["history"].numpy()
        try:
            pol.latent_saliency(**call)
            raise AssertionError(("accepted", kw))
        except ValueError as e:
            assert "latent_saliency" in str(e), (kw, str(e))
    from iplan_amd.nova import behavior_FC_policy, behavior_policy
    for mod, kw in ((behavior_policy, {}), (behavior_FC_policy, dict(behavior_fully_connected=True))):
        other = BC._policy(BC._e2e_args(device, **kw), 41, cls=mod.Behavior_policy)
        try:
            other.latent_saliency(hist.numpy())
            raise AssertionError("accepted")
        except NotImplementedError as e:
            assert "soft-update" in str(e), str(e)
    long_args = BC._e2e_args(device, max_history_len=L.ENC_SAL_MAX_L + 1, episode_limit=L.ENC_SAL_MAX_L + 4)
    long_pol = BC._policy(long_args, 43)
    try:
        long_pol.latent_saliency(np.zeros((1, L.ENC_SAL_MAX_L + 4, nA, N, d)))
        raise AssertionError("a window longer than the kernel's limit was accepted")
    except NotImplementedError as e:
        assert "max_history_len" in str(e), str(e)
    return {}


def check_window_lengths(device, lengths=(3, 12, 16, L.ENC_SAL_MAX_L)):
    """L up to the kernel's limit works; the number of waves per workgroup follows from L (here 4, 2, 1, 1; the cases' L = 10 has 3):
    against fp64 at one full tile and a ragged second"""
    worst = {}
    for Lw in lengths:
        case = Case(1, 17, 5, 8, Lw, 3, 1, device, seed=Lw)
        out = case.run((0, 2), 1, "argmax")
        v = case.cotangent(out, (0, 2), "argmax", None)
        assert_vs_fp64(case, out, case.references(out, (0, 2), 1, v), worst, ("L", Lw))
        assert_structure(case, out, (0, 2), 1)
    return worst
