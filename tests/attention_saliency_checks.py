"""TEST INFRASTRUCTURE: attention saliency (csrc/gat_saliency.hip, ops.gat_saliency, Prediction_policy.attention_saliency) on whatever
library is active -- the host emulator in tests/test_emu_attention_saliency.py, the gfx950 build in tests/test_gpu_attention_saliency.py.

Ground truth: fp64 torch.autograd.grad through oracle.gat_forward on the same inputs.  y_i = <v_i, latent_i> is differentiated one
ego at a time: the scene is replicated N times along the oracle's batch axis and copy i contributes <v_i, latent[copy i, ego i]>, so
one backward pass gives G[i] = d y_i / d obs[copy i] for every ego.  Both ReLUs of the oracle take the branch the kernel took (its
``active_h`` / ``active_v``), and ``gate="held"`` detaches the gumbel gate -- both by wrapping torch.relu /
torch.softmax for the duration of the oracle call (gat_forward calls each exactly twice, in a fixed order).
Bounds: at tau = 1 and 0.25 every tensor within 1e-5 of the fp64 tensor's own maximum; at the shipped tau = 0.01
max(1e-5, E32_FACTOR x e32) relative to max(1, |ref|), e32 = the fp32 oracle's own error against fp64, after asserting e32 <= 1e-4.
The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors it saw."""
import contextlib
import functools
from unittest import mock

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.kernel_checks import _sentinel
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5
E32_CAP = 1e-4
A = 32
OUTS = ("grad", "pair_gl1", "pair_gxi", "input_grad", "hidden_grad")
# (n_nets, B, N, d0, d1, tau, gate, target, noise)
EDGE_N_EMU = (2, 3, 15, 16, 17, 33)
EDGE_N_GPU = (32, 48, 49, 63, 64)


def kernel_cases(sizes):
    cases = [(1, 2, N, 5, 8, 1.0, "through", "tensor", True) for N in sizes]
    if 17 in sizes:
        cases += [(1, 1, 17, d0, d1, 1.0, "through", "tensor", True) for d0, d1 in ((1, 0), (5, 1), (64, 64))]
        cases += [(2, 1, 5, 5, 8, 1.0, "through", "tensor", True), (5, 1, 3, 5, 8, 0.25, "through", "self", True)]
        cases += [(1, 1, N, 5, 8, 0.25, "through", "tensor", True) for N in (3, 17)]
        cases += [(1, 1, N, 5, 8, tau, "held", "tensor", True) for N, tau in ((2, 1.0), (3, 0.25), (17, 1.0), (33, 0.25))]
        cases += [(1, 1, 17, 5, 8, 1.0, "through", "self", True), (1, 1, 17, 5, 8, 0.25, "through", 7, True),
                  (1, 1, 17, 5, 8, 1.0, "through", "tensor", False), (1, 1, 17, 5, 8, 0.25, "held", "self", False)]
    else:
        cases += [(1, 1, 64, 5, 8, 0.25, "held", "self", False), (2, 1, 49, 5, 0, 0.25, "through", 3, True)]
    return cases


def case_id(c):
    n, B, N, d0, d1, tau, gate, target, noise = c
    return f"n{n}_B{B}_N{N}_d{d0}+{d1}_tau{tau}_{gate}_{target}_{'noise' if noise else 'nonoise'}"


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _gumbel(gen, *shape):
    u = torch.rand(*shape, generator=gen).clamp_min(1e-20)
    return -torch.log((-torch.log(u)).clamp_min(1e-20))


# ------------------------------------------------------------------------------------------------ the fp64 / fp32 judge
@contextlib.contextmanager
def _pinned(active_h, active_v, held):
    """oracle.gat_forward with the two ReLUs on the given branches (bool tensors shaped like their arguments) and, if ``held``, the
    gumbel gate (the first of its two softmax calls) detached"""
    real_relu, real_softmax = torch.relu, torch.softmax
    relu_calls, softmax_calls = [], []

    def relu(z):
        mask = (active_h, active_v)[len(relu_calls)]
        relu_calls.append(1)
        return z * mask.to(z.dtype)

    def softmax(z, dim=-1):
        softmax_calls.append(1)
        out = real_softmax(z, dim=dim)
        return out.detach() if held and len(softmax_calls) == 1 else out

    with mock.patch.object(torch, "relu", relu), mock.patch.object(torch, "softmax", softmax):
        yield
    assert len(relu_calls) == 2 and len(softmax_calls) == 2, (len(relu_calls), len(softmax_calls))


def reference_scene(p, obs, hprev, noise, v, tau, active_h, active_v, held, dtype):
    """one scene: p = GAT state dict, obs [N, D], hprev [N, A], noise [N, N-1, 2], v [N, A] (a constant), active_* [N, 32] bool ->
    dict of latent [N, A], grad [N, N, D], hidden_grad [N, A] in ``dtype``"""
    N = obs.shape[0]
    p = {k: t.to(dtype) for k, t in p.items()}
    rep = lambda t: t.to(dtype)[None].expand(N, *t.shape).clone()                 # noqa: E731
    obs_r, h_r = rep(obs).requires_grad_(True), rep(hprev).requires_grad_(True)
    mh, mv = active_h[None].expand(N, N, A), active_v[None].expand(N, N, A)
    with _pinned(mh, mv, held):
        out = O.gat_forward(p, obs_r, h_r.reshape(N * N, A), rep(noise).reshape(-1, 2), tau=tau).view(N, N, A)
    idx = torch.arange(N)
    y = (v.to(dtype) * out[idx, idx]).sum()
    G, gh = torch.autograd.grad(y, (obs_r, h_r))
    return dict(latent=out[0].detach(), grad=G, hidden_grad=gh[idx, idx])


def derived(grad, obs, d0):
    """grad [..., N, N, D], obs [..., N, D] -> pair_gl1, pair_gxi [..., N, N, n_src], input_grad [..., N, D] in grad's dtype"""
    D = grad.shape[-1]
    cuts = [(0, d0)] + ([(d0, D)] if D > d0 else [])
    gx = grad * obs.to(grad.dtype)[..., None, :, :]
    return dict(pair_gl1=torch.stack([grad[..., lo:hi].abs().sum(-1) for lo, hi in cuts], -1),
                pair_gxi=torch.stack([gx[..., lo:hi].sum(-1) for lo, hi in cuts], -1), input_grad=grad.sum(-3))


class Case:
    """default-initialised GAT nets (the last one ends the arena), inputs in [-1, 1]; src0 / src1 are env-major strided views
    [n, B, N, d] of buffers [B, n, N d + pad] with guard floats in front of and behind every scene's block"""

    def __init__(self, n, B, N, d0, d1, device, seed=0):
        from iplan_amd.arena import ParamArena
        from iplan_amd.config import default_args
        from iplan_amd.nova.GAT_Net import GAT_Net
        self.dims, self.device = (n, B, N, d0, d1), device
        torch.manual_seed(11 + 1000 * n + 100 * B + N + d0 + d1 + seed)
        args = default_args("highway", use_cuda=False)
        self.mods = [GAT_Net(d0 + d1, args) for _ in range(n)]
        self.params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.mods]
        self.arena = ParamArena(self.mods, device)
        gen = torch.Generator().manual_seed(seed + n + B + N)
        self.buf0 = torch.rand(B, n, N * d0 + 5, generator=gen) * 2 - 1
        self.buf1 = torch.rand(B, n, N * max(d1, 1) + 3, generator=gen) * 2 - 1
        self.hidden = torch.randn(n, B, N, A, generator=gen) * 0.1
        self.noise = _gumbel(gen, n, B, N, N - 1, 2)
        self.v = torch.randn(n, B, N, A, generator=gen)
        self.upload()

    def _view(self, buf, d, lead):
        N = self.dims[2]
        return buf[:, :, lead:lead + N * d].unflatten(-1, (N, d)).permute(1, 0, 2, 3)          # [n, B, N, d], env-major

    def upload(self):
        dev = self.device
        n, B, N, d0, d1 = self.dims
        self.src0, self.src1 = self._view(self.buf0, d0, 2), (self._view(self.buf1, d1, 1) if d1 else None)
        self.d_buf0, self.d_buf1 = self.buf0.to(dev), self.buf1.to(dev)
        self.d_src0, self.d_src1 = self._view(self.d_buf0, d0, 2), (self._view(self.d_buf1, d1, 1) if d1 else None)
        assert self.d_src0.stride(0) <= self.d_src0.stride(1)
        self.d_hidden, self.d_noise, self.d_v = self.hidden.to(dev), self.noise.to(dev), self.v.to(dev)

    def obs(self):
        return self.src0 if self.src1 is None else torch.cat([self.src0, self.src1], -1)

    def forward(self, tau, noise=True, scenes=None):
        """the training-form forward of the scenes ``scenes`` (a slice over B): (latent, saved)"""
        sl = slice(None) if scenes is None else scenes
        nz = self.d_noise[:, sl].contiguous() if noise else torch.zeros_like(self.d_noise[:, sl])
        return ops.gat_forward(self.arena, self.d_src0[:, sl], None if self.d_src1 is None else self.d_src1[:, sl], self.d_hidden[:, sl], nz,
                               tau=tau, save=True)

    def target(self, kind, latent, scenes=None):
        if isinstance(kind, str) and kind == "self":
            return latent
        if isinstance(kind, int):
            t = torch.zeros_like(latent)
            t[..., kind] = 1.0
            return t
        return self.d_v if scenes is None else self.d_v[:, scenes]

    def run(self, tau=1.0, gate="through", target="tensor", noise=True, want=OUTS, out=None, scenes=None, v=None, poison=False):
        latent, saved = self.forward(tau, noise, scenes)
        vt = self.target(target, latent, scenes) if v is None else v
        if poison:
            saved["gru"].fill_(float("nan"))
        res = dict(ops.gat_saliency(self.arena, saved, vt, gate_through=gate == "through", want=want, out=out))
        _sync(self.device)
        n, B, N = latent.shape[:3]
        res.update(latent=latent, v=vt, active_h=saved["h_enc"].view(n, B, N, A) > 0, active_v=saved["qkv"].view(n, B, N, 3 * A)[..., 2 * A:] > 0)
        res.pop("_keep")
        return res

    def reference(self, got, dtype, tau, gate, noise):
        """the judge on the kernel's own v and ReLU branches: dict of [n, B, ...] tensors in ``dtype``"""
        n, B, N, d0, d1 = self.dims
        obs = self.obs()
        v, ah, av = got["v"].cpu(), got["active_h"].cpu(), got["active_v"].cpu()
        rows = {k: [] for k in ("latent", "grad", "hidden_grad")}
        for i in range(n):
            per = {k: [] for k in rows}
            for b in range(B):
                nz = self.noise[i, b] if noise else torch.zeros(N, N - 1, 2)
                r = reference_scene(self.params[i], obs[i, b], self.hidden[i, b], nz, v[i, b], tau, ah[i, b], av[i, b], gate == "held", dtype)
                for k in per:
                    per[k].append(r[k])
            for k in rows:
                rows[k].append(torch.stack(per[k]))
        ref = {k: torch.stack(t) for k, t in rows.items()}
        ref.update(derived(ref["grad"], obs, d0))
        return ref


@functools.lru_cache(maxsize=8)
def get_case(dims, device, seed=0):
    return Case(*dims, device, seed=seed)


# ------------------------------------------------------------------------------------------------ 1: the kernel against fp64
def check_kernel(device, n, B, N, d0, d1, tau, gate, target, noise):
    case = get_case((n, B, N, d0, d1), device)
    got = case.run(tau, gate, target, noise)
    ref = case.reference(got, torch.float64, tau, gate, noise)
    worst = {}
    for k in OUTS + ("latent",):
        err = _grad_err(got[k], ref[k])
        print(case_id((n, B, N, d0, d1, tau, gate, target, noise)), k, "err", err)
        _worse(worst, f"{k}_tau{tau}", err)
    for k in OUTS + ("latent",):
        assert worst[f"{k}_tau{tau}"] <= TOL, (k, worst)
    if N == 2 and gate == "held":
        # the softmax over ONE neighbour is the constant 1: no d score, and with the gate held nothing else reaches the ego's own row
        g = got["grad"].cpu()
        assert torch.equal(g[:, :, 0, 0], torch.zeros_like(g[:, :, 0, 0])) and torch.equal(g[:, :, 1, 1], torch.zeros_like(g[:, :, 1, 1])), \
            "N = 2, held gate: the ego's own row is not exactly 0"
        assert g[:, :, 0, 1].abs().max() > 0
    return worst


# ------------------------------------------------------------------------------------------------ 2: the shipped tau
def check_shipped_tau(device, n, B, N, noise, d0=5, d1=8, tau=0.01):
    case = get_case((n, B, N, d0, d1), device, 1)
    got = case.run(tau, "through", "tensor", noise)
    r64 = case.reference(got, torch.float64, tau, "through", noise)
    r32 = case.reference(got, torch.float32, tau, "through", noise)
    worst = {}

    def rel(x, ref):
        return (x.double().cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())

    for k in OUTS + ("latent",):
        e32, err = rel(r32[k], r64[k]), rel(got[k], r64[k])
        print("tau", tau, "N", N, "noise", noise, k, "err", err, "e32", e32, "max|ref|", r64[k].abs().max().item())
        _worse(worst, f"{k}_tau{tau}", err)
        _worse(worst, f"{k}_tau{tau}_e32", e32)
        assert e32 <= E32_CAP, (k, "the fp32 oracle itself is off by", e32)
        assert err <= max(TOL, E32_FACTOR * e32), (k, err, e32)
    return worst


# ------------------------------------------------------------------------------------------------ 3: exact statements
def _same(a, b, what, keys=OUTS + ("latent",)):
    for k in keys:
        if k in a and k in b:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def check_exact(device, N=17, n=2, B=3, tau=0.25):
    case = get_case((n, B, N, 5, 8), device, 2)
    full = case.run(tau)
    # input_grad = the running fp32 sum of G over the egos, ascending
    g = full["grad"].cpu()
    acc = torch.zeros_like(g[:, :, 0])
    for i in range(N):
        acc = acc + g[:, :, i]
    assert torch.equal(full["input_grad"].cpu(), acc), "input_grad is not the ascending fp32 sum of grad over the egos"
    _same(case.run(tau), full, "a second launch")
    for wanted in (("input_grad",), ("pair_gl1", "pair_gxi", "hidden_grad"), ("grad",)):
        _same(case.run(tau, want=wanted), full, f"want={wanted}")
    for b in range(B):                                                         # alone == inside the batch
        one = case.run(tau, scenes=slice(b, b + 1))
        _same(one, {k: full[k][:, b:b + 1] for k in OUTS + ("latent",)}, f"scene {b} alone")
    # ... and at another position: the batch with its scenes reversed
    rev = Case(n, B, N, 5, 8, device, seed=2)
    for name in ("buf0", "buf1", "hidden", "noise", "v"):
        t = getattr(case, name)
        setattr(rev, name, t.flip(0 if name.startswith("buf") else 1).contiguous())
    rev.params, rev.arena = case.params, case.arena
    rev.upload()
    _same(rev.run(tau), {k: full[k].flip(1) for k in OUTS + ("latent",)}, "scenes at other positions")
    # an ego with v_i = 0: exact zeros
    v = case.d_v.clone()
    v[:, :, 3] = 0.0
    z = case.run(tau, v=v)
    for k in ("grad", "pair_gl1", "pair_gxi", "hidden_grad"):
        row = z[k][:, :, 3].cpu()
        assert torch.equal(row, torch.zeros_like(row)), (k, "of an ego with v = 0 is not exactly 0")
    assert z["grad"][:, :, 4].abs().max() > 0
    # a held gate never reads the pair-GRU record
    held = case.run(tau, gate="held")
    poisoned = case.run(tau, gate="held", poison=True)
    for k in OUTS:
        assert torch.isfinite(poisoned[k]).all(), (k, "read the poisoned pair-GRU record")
    _same(poisoned, held, "held gate with the record poisoned")
    assert not torch.equal(held["grad"], full["grad"])
    return {}


# ------------------------------------------------------------------------------------------------ 4: linearity in the cotangent
def check_linearity(device, N=17, tau=1.0, alpha=0.75, beta=-1.5):
    case = get_case((1, 1, N, 5, 8), device, 3)
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(case.v.shape, generator=gen)
    vs = {"v": case.v, "w": w, "mix": alpha * case.v + beta * w}
    got = {k: case.run(tau, v=t.to(device)) for k, t in vs.items()}
    obs = case.obs()

    def lin_err(G):
        comb = alpha * G["v"] + beta * G["w"]                                  # the fp32 rounding of the sum is part of the statement
        return _grad_err(comb, G["mix"])

    o32 = {}
    for k, t in vs.items():
        o32[k] = reference_scene(case.params[0], obs[0, 0], case.hidden[0, 0], case.noise[0, 0], t[0, 0], tau, got["mix"]["active_h"][0, 0].cpu(),
                                 got["mix"]["active_v"][0, 0].cpu(), False, torch.float32)["grad"]
    e_oracle = lin_err(o32)
    e_kernel = lin_err({k: r["grad"][0, 0].cpu() for k, r in got.items()})
    print("linearity: kernel", e_kernel, "fp32 oracle", e_oracle)
    assert e_oracle > 0
    assert e_kernel <= E32_FACTOR * e_oracle, (e_kernel, e_oracle)
    return {"linearity": e_kernel, "linearity_e32": e_oracle}


# ------------------------------------------------------------------------------------------------ 5: ownership
def check_ownership(device, n=2, B=2, N=17, tau=0.25):
    case = get_case((n, B, N, 5, 8), device, 4)
    ref = case.run(tau)
    D, n_src = 13, 2
    shapes = {"grad": (N, N, D), "pair_gl1": (N, N, n_src), "pair_gxi": (N, N, n_src), "input_grad": (N, D), "hidden_grad": (N, A)}

    def carve(k, shift=0.0):
        inner = int(np.prod(shapes[k]))
        pad = 7 if k.startswith("pair") else 5                                # the two pair maps share their strides
        total = n * B * (inner + pad) + 64
        sent = _sentinel(total) + shift
        buf = sent.clone().to(device)
        view = buf[32:32 + n * B * (inner + pad)].view(n, B, inner + pad)[:, :, :inner].unflatten(-1, shapes[k])
        mask = torch.ones(total, dtype=torch.bool)
        mask[32:32 + n * B * (inner + pad)].view(n, B, inner + pad)[:, :, :inner] = False
        return sent, buf, view, mask

    for wanted in (OUTS, ("input_grad",), ("pair_gl1", "pair_gxi")):
        bufs = {k: carve(k) for k in shapes}
        got = case.run(tau, want=wanted, out={k: bufs[k][2] for k in wanted})
        for k, (sent, buf, view, mask) in bufs.items():
            host = buf.cpu()
            if k not in wanted:
                assert torch.equal(host.view(torch.int32), sent.view(torch.int32)), (k, "was not asked for and was written")
                continue
            assert got[k].data_ptr() == view.data_ptr()
            assert torch.equal(_bits(view), _bits(ref[k])), (k, "differs inside a padded buffer")
            assert torch.equal(host[mask].view(torch.int32), sent[mask].view(torch.int32)), (k, "a float outside the owned views was written")
    b2 = {k: carve(k, 0.25) for k in shapes}                                  # every owned float is written
    case.run(tau, out={k: b2[k][2] for k in shapes})
    for k in shapes:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (k, "an owned float was left unwritten")
    # NaN around the inputs: the guard floats of the source buffers, and v as a view into a NaN-filled buffer
    keep0, keep1 = case.buf0.clone(), case.buf1.clone()
    try:
        for buf, lead, d in ((case.buf0, 2, 5), (case.buf1, 1, 8)):
            buf[:, :, :lead] = float("nan")
            buf[:, :, lead + N * d:] = float("nan")
        case.upload()
        vbuf = torch.full((n, B, N * A + 8), float("nan"), device=device)
        vv = vbuf[:, :, 4:4 + N * A].unflatten(-1, (N, A))
        vv.copy_(case.d_v)
        _same(case.run(tau, v=vv), ref, "NaN around the inputs")
    finally:
        case.buf0.copy_(keep0)
        case.buf1.copy_(keep1)
        case.upload()
    return {}


# ------------------------------------------------------------------------------------------------ the method
def _policy(device, seed=17, **kw):
    from iplan_amd.config import default_args
    from iplan_amd.nova.prediction_policy import Prediction_policy
    base = dict(use_cuda=torch.device(device).type == "cuda", max_vehicle_num=5, n_agents=2, episode_limit=12, pred_length=3, pred_batch_size=6)
    base.update(kw)
    args = default_args("highway", **base)
    torch.manual_seed(seed)
    pol = Prediction_policy(args, _Log())
    gat = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in pol.pred_GAT]
    return args, pol, gat


def _method_reference(gat, hist, lat, hid, noise, got, tau, gate, dtype):
    """every row of the method's result through the judge: dict of [E, S, nA, ...]"""
    E, S, nA, N, d = hist.shape
    obs = torch.cat([hist, lat], -1) if lat is not None else hist
    keys = ("latent", "grad", "hidden_grad")
    out = {k: torch.zeros(E, S, nA, *shape, dtype=dtype) for k, shape in (("latent", (N, A)), ("grad", (N, N, obs.shape[-1])), ("hidden_grad", (N, A)))}
    cpu = {k: torch.as_tensor(got[k]).cpu() for k in ("target_vector", "active_h", "active_v")}
    for e in range(E):
        for s in range(S):
            for i in range(nA):
                nz = noise[i, e, s] if noise is not None else torch.zeros(N, N - 1, 2)
                r = reference_scene(gat[i], obs[e, s, i], hid[e, s, i], nz, cpu["target_vector"][e, s, i], tau, cpu["active_h"][e, s, i],
                                    cpu["active_v"][e, s, i], gate == "held", dtype)
                for k in keys:
                    out[k][e, s, i] = r[k]
    out.update(derived(out["grad"], obs, d))
    return out


def check_methods(device, E=2, S=2):
    """numpy and tensor inputs, types and shapes, values against fp64 at an overridden tau, chunked == unchunked, the latent's bits are
    attention_map's, the deterministic mode draws nothing"""
    args, pol, gat = _policy(device)
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    D = d + Z
    gen = torch.Generator().manual_seed(5)
    hist = torch.rand(E, S, nA, N, d, generator=gen) * 2 - 1
    lat = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
    hid = torch.randn(E, S, nA, N, A, generator=gen) * 0.1
    noise = _gumbel(gen, nA, E, S, N, N - 1, 2)
    tgt = torch.randn(E, S, nA, N, A, generator=gen)
    worst = {}
    to = lambda t: t.to(device)                                               # noqa: E731
    want = ("pair", "grad")
    shapes = {"pair_gl1": (N, N, 2), "pair_gxi": (N, N, 2), "grad": (N, N, D), "input_grad": (N, D), "hidden_grad": (N, A), "latent": (N, A),
              "target_vector": (N, A), "active_h": (N, A), "active_v": (N, A)}
    for tau, gate, target, nz in ((0.25, "through", tgt, noise), (1.0, "held", "self", None), (0.25, "through", 5, None)):
        kw = dict(hidden=to(hid), target=to(target) if torch.is_tensor(target) else target, gate=gate, tau=tau, want=want)
        if nz is not None:
            kw.update(noise=to(nz), deterministic=False)
        res = pol.attention_saliency(to(hist), to(lat), **kw)
        _sync(device)
        assert set(res) == set(shapes), set(res) ^ set(shapes)
        for k, shape in shapes.items():
            assert torch.is_tensor(res[k]) and res[k].shape == (E, S, nA) + shape and res[k].device.type == torch.device(device).type, (k, res[k].shape)
            assert res[k].dtype == (torch.bool if k.startswith("active") else torch.float32)
        ref = _method_reference(gat, hist, lat, hid, nz, res, tau, gate, torch.float64)
        for k in OUTS + ("latent",):
            err = _grad_err(res[k], ref[k])
            _worse(worst, "method_" + k, err)
            assert err <= TOL, (k, tau, gate, err)
        small = pol.attention_saliency(to(hist), to(lat), max_workspace_mb=0.3, **kw)          # one row per chunk
        _sync(device)
        for k in shapes:
            assert torch.equal(_bits(small[k]), _bits(res[k])), (k, "chunked differs from unchunked")
        few = pol.attention_saliency(to(hist), to(lat), **dict(kw, want=()))
        assert set(few) == set(shapes) - {"pair_gl1", "pair_gxi", "grad"}
        for k in few:
            assert torch.equal(_bits(few[k]), _bits(res[k])), (k, "depends on what else was asked for")
    # numpy in -> numpy out (float64 histories, as the runner hands them over)
    res_np = pol.attention_saliency(hist.double().numpy(), lat.numpy(), hidden=hid.numpy(), target=tgt.numpy(), tau=0.25, want=want)
    res_t = pol.attention_saliency(to(hist), to(lat), hidden=to(hid), target=to(tgt), tau=0.25, want=want)
    for k in shapes:
        assert isinstance(res_np[k], np.ndarray) and np.array_equal(res_np[k], res_t[k].cpu().numpy()), k
    # hidden=None is zeros
    zero = pol.attention_saliency(to(hist), to(lat), hidden=torch.zeros_like(hid).to(device))
    none = pol.attention_saliency(to(hist), to(lat))
    for k in none:
        assert torch.equal(_bits(none[k]), _bits(zero[k])), (k, "hidden=None != zeros")
    # the latent is attention_map's, bit for bit, at the policy's own tau -- without noise and with it; the former draws nothing
    states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None)
    det = pol.attention_saliency(to(hist), to(lat), hidden=to(hid))
    assert torch.equal(torch.get_rng_state(), states[0])
    if states[1] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), states[1])
    noisy = pol.attention_saliency(to(hist), to(lat), hidden=to(hid), noise=to(noise), deterministic=False)
    own = pol.attention_saliency(to(hist), to(lat), hidden=to(hid), deterministic=False)
    assert torch.isfinite(own["input_grad"]).all()
    for s in range(S):
        m0 = pol.attention_map(to(hist[:, s]), to(hid[:, s]), to(lat[:, s]), deterministic=True)
        m1 = pol.attention_map(to(hist[:, s]), to(hid[:, s]), to(lat[:, s]), noise=to(noise[:, :, s].contiguous()))
        _sync(device)
        assert torch.equal(_bits(det["latent"][:, s]), _bits(m0["latent"])), "latent != attention_map's (deterministic)"
        assert torch.equal(_bits(noisy["latent"][:, s]), _bits(m1["latent"])), "latent != attention_map's (with noise)"
    return worst


# ------------------------------------------------------------------------------------------------ 6: the chain with the policy
def check_chain(device, dims=(2, 1, 2, 3, 5)):
    """d log pi(a*) / d [history || behavior_latent] in total = the policy's own hist / beh columns + attention_saliency's input_grad
    seeded with the policy's att columns, against fp64 autograd through oracle.gat_forward -> build_inputs_train -> actor_evaluate
    with the recorded GRU state and the attention ``hidden`` held fixed"""
    from iplan_amd import synth
    from iplan_amd.nova.prediction_policy import Prediction_policy
    from tests import saliency_checks as SC
    from tests.policy_trace_checks import _params
    nA, E, S, N, d = dims
    case = SC.Case(dims, device, seed=3)
    a, f = case.args, case.f
    Z, M = a.latent_dim, a.rnn_hidden_dim
    torch.manual_seed(23)
    pol = Prediction_policy(a, _Log())
    gat = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in pol.pred_GAT]
    gen = torch.Generator().manual_seed(8)
    hist = (torch.rand(E, S, nA, N, d, generator=gen) * 2 - 1)
    beh = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
    hid = torch.randn(E, S, nA, N, A, generator=gen) * 0.1
    tau = 0.25
    first = pol.attention_saliency(hist.to(device), beh.to(device), hidden=hid.to(device), tau=tau, want=())
    # the policy sees exactly this latent as its att columns
    f = dict(f)
    f["history"] = torch.cat([hist, f["history"][:, S:]], 1)
    f["behavior_latent"] = torch.cat([beh, f["behavior_latent"][:, S:]], 1)
    f["attention_latent"] = torch.cat([first["latent"].cpu(), f["attention_latent"][:, S:]], 1)
    batch = synth.DictBatch(f, E, S + 1).to(device)
    sal = case.mac.saliency(batch, target="recorded", which="actor", want=("input_grad", "act"), steps=slice(0, S))
    W = d + A + Z
    ent = sal["actor_input_grad"][..., :N * W].reshape(E, S, nA, N, W)
    res = pol.attention_saliency(hist.to(device), beh.to(device), hidden=hid.to(device), target=ent[..., d:d + A].contiguous(), tau=tau, want=())
    _sync(device)
    assert torch.equal(_bits(res["latent"]), _bits(first["latent"]))
    total = res["input_grad"].cpu() + torch.cat([ent[..., :d], ent[..., d + A:]], -1).cpu()
    ap, _ = _params(case.mac, torch.float64)
    ref = torch.zeros(E, S, nA, N, d + Z, dtype=torch.float64)
    ah, av = res["active_h"].cpu(), res["active_v"].cpu()
    n_act = a.n_actions
    for i in range(nA):
        h_leaf = hist[:, :, i].double().clone().requires_grad_(True)
        b_leaf = beh[:, :, i].double().clone().requires_grad_(True)
        obs = torch.cat([h_leaf, b_leaf], -1).reshape(E * S, N, d + Z)
        p = {k: t.double() for k, t in gat[i].items()}
        with _pinned(ah[:, :, i].reshape(E * S, N, A), av[:, :, i].reshape(E * S, N, A), False):
            att = O.gat_forward(p, obs, hid[:, :, i].double().reshape(E * S * N, A), torch.zeros(E * S * N * (N - 1), 2, dtype=torch.float64), tau=tau)
        x = O.build_inputs_train(i, h_leaf, att.view(E, S, N, A), b_leaf, torch.zeros(E, S, n_act, dtype=torch.float64), nA, a.GAT_enable,
                                 a.Behavior_enable)
        acts = f["actions"][:, :S, i, 0]
        parts = [x[..., :x.shape[-1] - n_act - nA]]
        last = torch.cat([torch.full_like(acts[:, :1], -1), acts[:, :-1]], 1)
        oh = torch.zeros(E, S, n_act, dtype=torch.float64)
        oh.scatter_(-1, last.clamp_min(0).unsqueeze(-1), (last >= 0).double().unsqueeze(-1))
        idoh = torch.zeros(E, S, nA, dtype=torch.float64)
        idoh[..., i] = 1
        x = torch.cat(parts + [oh, idoh], -1).reshape(E * S, -1)
        hints = (sal["actor_act1"][:, :, i].reshape(E * S, M).cpu() > 0, sal["actor_act2"][:, :, i].reshape(E * S, M).cpu() > 0)
        logp, _ = O.actor_evaluate(ap[i], x, f["rnn_states_actors"][:, :S, i].reshape(E * S, M).double(), acts.reshape(-1),
                                   f["avail_actions"][:, :S, i].reshape(E * S, -1), relu_hint=hints, use_relu=a.use_ReLU)
        gh, gb = torch.autograd.grad(logp.sum(), (h_leaf, b_leaf))
        ref[:, :, i] = torch.cat([gh, gb], -1)
        assert _grad_err(sal["logp"][:, :, i].cpu(), logp.detach().view(E, S)) <= TOL
    err = _grad_err(total, ref)
    through_gat = _grad_err(res["input_grad"].cpu(), torch.zeros_like(ref))
    print("chain: err", err, "share that went through the GAT", res["input_grad"].abs().max().item() / ref.abs().max().item())
    assert through_gat > 0 and err <= TOL, err
    return {"chain": err}


# ------------------------------------------------------------------------------------------------ 7: touches nothing
def check_touches_nothing(device, E=2):
    from iplan_amd import synth
    from iplan_amd.nova.prediction_policy import Prediction_policy
    args, pol, _ = _policy(device)
    nA, N, P, S = args.n_agents, args.max_vehicle_num, args.pred_length, args.pred_batch_size
    batch = synth.make_batch(args, E, seed=9, terminated_p=0.1, device=device)
    D = batch.data
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), ggrad=pol.gat_arena.grad.clone(), dgrad=pol.dec_arena.grad.clone(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer], rng=torch.get_rng_state(),
                  crng=torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, vars=sorted(vars(pol)))
    res = pol.attention_saliency(D["history"][:, 1:4], D["behavior_latent"][:, :3], hidden=D["attention_latent"][:, :3], want=("pair", "grad"))
    _sync(device)
    assert torch.isfinite(res["grad"]).all()
    assert torch.equal(pol.gat_arena.data, before["gat"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert torch.equal(_bits(pol.gat_arena.grad), _bits(before["ggrad"])) and torch.equal(_bits(pol.dec_arena.grad), _bits(before["dgrad"]))
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"] and sorted(vars(pol)) == before["vars"]
    assert torch.equal(torch.get_rng_state(), before["rng"])
    if before["crng"] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), before["crng"])
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
            p2.attention_saliency(D["history"][:, 1:3], D["behavior_latent"][:, :2], hidden=D["attention_latent"][:, :2], gate="held")
        losses = p2.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), p2.gat_arena.data.clone(), p2.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


# ------------------------------------------------------------------------------------------------ 8: refusals
def _codes():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iplan_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"(IPLAN_E\w+)\s*=\s*(-?\d+)", text)}
    return vals["IPLAN_EINVAL"], vals["IPLAN_EALIGN"]


def check_entry_point_refusals(device):
    """each of these is refused with its code and a message, without a launch"""
    case = get_case((1, 1, 5, 5, 8), device, 6)
    good = case.run()
    lib = ops._lib(None)
    latent, saved = case.forward(1.0)
    a, res, keep = ops.gat_saliency_args(case.arena, saved, case.d_v, True, OUTS)
    EINVAL, EALIGN = _codes()

    def get(obj, path):
        for name in path.split(".")[:-1]:
            obj = getattr(obj, name)
        return obj, path.split(".")[-1]

    def refused(code, **fields):
        fields = {k.replace("__", "."): v for k, v in fields.items()}
        old = {}
        for k, v in fields.items():
            o, name = get(a, k)
            old[k] = getattr(o, name)
            setattr(o, name, v)
        rc = lib.c.iplan_gat_saliency(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, v in old.items():
            o, name = get(a, k)
            setattr(o, name, v)
        assert rc == code and "iplan_gat_saliency" in msg, (fields, rc, msg)

    assert lib.c.iplan_gat_saliency(None, L.C.c_void_p(0)) == EINVAL
    refused(EINVAL, fwd__N=1)
    refused(EINVAL, fwd__N=65)
    refused(EINVAL, fwd__n_nets=0)
    refused(EINVAL, fwd__B=0)
    refused(EINVAL, fwd__d0=0)
    refused(EINVAL, fwd__d1=-1)
    refused(EINVAL, gate_through=2)
    refused(EINVAL, fwd__saved__cell=None)
    refused(EINVAL, fwd__saved__gru=None)
    refused(EINVAL, v=None)
    refused(EINVAL, fwd__src1=None)
    refused(EINVAL, grad=None, pair_gl1=None, pair_gxi=None, input_grad=None, hidden_grad=None)
    refused(EINVAL, fwd__tau=0.0)
    refused(EINVAL, scratch=None)
    refused(EINVAL, scratch_floats=a.scratch_floats - 1)
    refused(EALIGN, scratch=a.scratch + 4)
    lib.call("iplan_gat_saliency", a)                                          # the restored descriptor is accepted
    _sync(device)
    _same(res, good, "after the refusals", OUTS)
    # a held gate needs neither the record nor the scratch
    a.gate_through, a.scratch, a.scratch_floats = 0, None, 0
    a.fwd.saved.gru = None
    lib.call("iplan_gat_saliency", a)
    _sync(device)
    _same(res, case.run(gate="held"), "held gate without record and scratch", OUTS)
    del keep, latent
    return {}


def check_method_refusals(device):
    args, pol, _ = _policy(device)
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    E, S = 1, 2
    hist, lat = torch.rand(E, S, nA, N, d).to(device), torch.rand(E, S, nA, N, Z).to(device)

    def refused(*a, **kw):
        try:
            pol.attention_saliency(*a, **kw)
        except ValueError as e:
            assert "attention_saliency" in str(e), e
            return
        raise AssertionError(f"not refused: {kw}")

    refused(hist)                                                             # behavior_latent missing
    refused(hist[0], lat)
    refused(hist[..., :d - 1], lat)
    refused(hist, lat[..., :Z - 1])
    refused(hist, lat, hidden=torch.zeros(E, S, nA, N, A - 1))
    refused(hist, lat, target=torch.zeros(E, S, nA, N))
    refused(hist, lat, target="latent")
    refused(hist, lat, target=A)
    refused(hist, lat, target=1.5)
    refused(hist, lat, gate="soft")
    refused(hist, lat, want=("pair", "maps"))
    refused(hist, lat, noise=torch.zeros(nA, E, S, N, N - 1, 2))              # with deterministic=True
    refused(hist, lat, noise=torch.zeros(nA, E, S, N, N, 2), deterministic=False)
    refused(hist, lat, tau=0.0)
    refused(hist, lat, max_workspace_mb=0.001)
    assert torch.isfinite(pol.attention_saliency(hist, lat)["input_grad"]).all()
    return {}
