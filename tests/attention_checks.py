"""TEST INFRASTRUCTURE: attention inspection (csrc/gat_trace.hip, ops.gat_trace, Prediction_policy.attention_map / attention_trace)
on whatever library is active -- the host emulator in tests/test_emu_attention.py, the gfx950 build in tests/test_gpu_attention.py.

Ground truth: oracle.gat_forward(..., return_internals=True) stepped S times, in fp64 and in fp32.  Rule (tests/oracle_checks.py):
error = max|got - ref64| / max|ref64| per tensor and step, bound = max(1e-5, E32_FACTOR x the fp32 oracle's own error against fp64 on
the same tensor at the same step) -- the tau = 0.01 gate and the closed loop over the steps make a flat 1e-5 unattainable for any fp32
arithmetic.  The six sums are compared with the same sums formed in fp64 from the fp64 oracle's soft / hard, under the same rule
relative to each sum (e32: the fp32 oracle's sums).  The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5
A = 32
# (n_nets, B, S, N, d0, d1)
KERNEL_CASES = [(1, 1, 1, 2, 5, 0), (2, 2, 3, 5, 5, 8), (1, 2, 2, 16, 5, 8), (1, 1, 3, 17, 5, 8), (2, 1, 2, 33, 5, 12), (1, 1, 2, 64, 4, 8),
                (5, 1, 4, 7, 5, 8)]
MAPS = ("soft", "hard", "attn")


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def _gumbel(gen, *shape):
    u = torch.rand(*shape, generator=gen).clamp_min(1e-20)
    return -torch.log((-torch.log(u)).clamp_min(1e-20))


def scatter(slot, N):
    """[..., N, N-1] slot-indexed -> [..., N, N] entity-indexed, diagonal 0: [i, j] = slot j - [j > i] of ego i"""
    out = torch.zeros(*slot.shape[:-1], N, dtype=slot.dtype)
    jidx = O.neighbour_index(N, "cpu")                                            # [N, N-1]: entity of slot s of ego i
    out.scatter_(-1, jidx.expand(*slot.shape[:-2], N, N - 1), slot)
    return out


class Case:
    """random GAT parameters; src0 / src1 are strided views [n, B, S, N, d] of larger episode-shaped buffers [B, S + 1, n, N + 1, d + 2]
    (so the net, env, step AND entity rows are not packed -- the entity stride must be d, so the view takes a packed [N, d] block out of
    a buffer whose other dims are padded); presence column 0 of src0 in {0, 1}"""

    def __init__(self, n, B, S, N, d0, d1, device, seed=0, presence_p=0.7):
        from iplan_amd.arena import ParamArena
        from iplan_amd.config import default_args
        from iplan_amd.nova.GAT_Net import GAT_Net
        self.dims = (n, B, S, N, d0, d1)
        self.device = device
        torch.manual_seed(7 + 1000 * n + 100 * B + 10 * S + N + d0 + d1 + seed)
        args = default_args("highway", use_cuda=False)
        self.mods = [GAT_Net(d0 + d1, args) for _ in range(n)]
        self.params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.mods]
        self.arena = ParamArena(self.mods, device)
        gen = torch.Generator().manual_seed(seed + n + B + S + N)
        self.buf0 = torch.rand(B, S + 1, n, N * d0 + 3, generator=gen) * 2 - 1
        self.buf1 = torch.softmax(torch.randn(B, S + 1, n, N * max(d1, 1) + 5, generator=gen), -1) * 4
        self.src0 = self._view(self.buf0, d0)
        self.src0[..., 0] = (torch.rand(n, B, S, N, generator=gen) < presence_p).float()
        self.src1 = self._view(self.buf1, d1) if d1 else None
        self.hidden0 = torch.randn(n, B, N, A, generator=gen) * 0.1
        self.noise = _gumbel(gen, n, B, S, N, N - 1, 2)
        self.weight = torch.randint(0, 4, (n, B, S), generator=gen).float() * 0.5
        self.upload()

    def _view(self, buf, d):
        n, B, S, N = self.dims[:4]
        return buf[:, 1:, :, 2:2 + N * d].unflatten(-1, (N, d)).permute(2, 0, 1, 3, 4)      # [n, B, S, N, d], nothing packed but [N, d]

    def upload(self):
        dev = self.device
        self.d_buf0, self.d_buf1 = self.buf0.to(dev), self.buf1.to(dev)
        d0, d1 = self.dims[4:]
        self.d_src0 = self._view(self.d_buf0, d0)
        self.d_src1 = self._view(self.d_buf1, d1) if d1 else None
        assert self.d_src0.untyped_storage().nbytes() > 4 * self.d_src0.numel()    # a view into a larger buffer, not a packed copy
        self.d_hidden0, self.d_noise, self.d_weight = self.hidden0.to(dev), self.noise.to(dev), self.weight.to(dev)

    def run(self, want=("latent",) + MAPS + ("stats",), noise=True, hidden0=True, weight=True, presence_col=0, out=None):
        res = ops.gat_trace(self.arena, self.d_src0, self.d_src1, self.d_hidden0 if hidden0 else None, self.d_noise if noise else None,
                            want=want, weight=self.d_weight if weight else None, presence_col=presence_col, out=out)
        _sync(self.device)
        return res

    def reference(self, dtype, noise=True, hidden0=True, weight=True, presence_col=0):
        """dict of latent [n,B,S,N,A], soft / hard / attn [n,B,S,N,N], stats [n,B,S,6] in ``dtype``"""
        n, B, S, N, d0, d1 = self.dims
        res = {k: [] for k in ("latent",) + MAPS + ("stats",)}
        for i in range(n):
            p = {k: v.to(dtype) for k, v in self.params[i].items()}
            h = (self.hidden0[i] if hidden0 else torch.zeros(B, N, A)).to(dtype).reshape(B * N, A)
            steps = {k: [] for k in res}
            for s in range(S):
                obs = self.src0[i, :, s] if not d1 else torch.cat([self.src0[i, :, s], self.src1[i, :, s]], -1)
                nz = (self.noise[i, :, s] if noise else torch.zeros(B, N, N - 1, 2)).to(dtype).reshape(-1, 2)
                h, it = O.gat_forward(p, obs.to(dtype), h, nz, return_internals=True)
                soft, hard = scatter(it["soft"], N), scatter(it["hard"], N)
                pres = (self.src0[i, :, s, :, presence_col] != 0).to(dtype) if presence_col >= 0 else torch.ones(B, N, dtype=dtype)
                off = 1 - torch.eye(N, dtype=dtype)
                pair = pres[:, :, None] * pres[:, None, :] * off
                w = (self.weight[i, :, s] if weight else torch.ones(B)).to(dtype)
                ent = -(torch.where(soft > 0, soft * torch.log(soft.clamp_min(1e-300)), torch.zeros_like(soft)) * off).sum(-1)
                st = torch.stack([pres.sum(-1), pair.sum((-1, -2)), (pair * hard).sum((-1, -2)), (pair * soft * hard).sum((-1, -2)),
                                  (pair * soft).sum((-1, -2)), (pres * ent).sum(-1)], -1) * w[:, None]
                for k, v in (("latent", h.reshape(B, N, A)), ("soft", soft), ("hard", hard), ("attn", soft * hard), ("stats", st)):
                    steps[k].append(v)
            for k in res:
                res[k].append(torch.stack(steps[k], 1))
        return {k: torch.stack(v) for k, v in res.items()}


def assert_vs_fp64(case, got, worst, what, **kw):
    r64, r32 = case.reference(torch.float64, **kw), case.reference(torch.float32, **kw)
    n, B, S = case.dims[:3]
    for k in ("latent",) + MAPS + ("stats",):
        if k not in got:
            continue
        g = got[k].cpu()
        for i in range(n):
            for s in range(S):
                if k == "stats":
                    for bb in range(B):
                        for c in range(6):                                        # each scene-step's sum relative to itself
                            ref = r64[k][i, bb, s, c:c + 1]
                            if ref.abs().max() == 0:
                                assert g[i, bb, s, c] == 0, (what, "stat", c, i, bb, s)
                                continue
                            e32, err = _grad_err(r32[k][i, bb, s, c:c + 1], ref), _grad_err(g[i, bb, s, c:c + 1], ref)
                            _worse(worst, f"stat{c}", err)
                            _worse(worst, f"stat{c}_e32", e32)
                            if _bound(e32) >= 0.1:
                                worst["loose_bounds"] = worst.get("loose_bounds", 0) + 1
                            assert err <= _bound(e32), (what, "stat", c, i, bb, s, err, e32)
                    continue
                e32, err = _grad_err(r32[k][i, :, s], r64[k][i, :, s]), _grad_err(g[i, :, s], r64[k][i, :, s])
                print(what, k, "net", i, "step", s, "err", err, "e32", e32)
                _worse(worst, k, err)
                _worse(worst, k + "_e32", e32)
                if _bound(e32) >= 0.1:                                            # (an fp32 gate flip at tau = 0.01: the bound says little there)
                    worst["loose_bounds"] = worst.get("loose_bounds", 0) + 1
                assert err <= _bound(e32), (what, k, i, s, err, e32)


# ------------------------------------------------------------------------------------------------ the kernel alone
def check_kernel(device, n, B, S, N, d0, d1):
    """every output at every step against fp64, with injected noise and with none; the layout properties on the way"""
    case = Case(n, B, S, N, d0, d1, device)
    worst = {}
    for noise in (True, False):
        got = case.run(noise=noise)
        assert_vs_fp64(case, got, worst, (n, B, S, N, d0, d1, "noise" if noise else "no noise"), noise=noise)
        soft, hard, attn = (got[k].cpu() for k in MAPS)
        eye = torch.eye(N, dtype=torch.bool)
        for m in (soft, hard, attn):
            assert torch.equal(m[..., eye], torch.zeros_like(m[..., eye])), "the diagonal is not exactly 0"
        assert torch.equal(attn.view(torch.int32), (soft * hard).view(torch.int32)), "attn != soft * hard bitwise"
    return worst


def check_same_bits_as_rollout(device, N, S=3, n=2, B=2, d0=5, d1=8):
    """latent[:, :, s] of ONE launch == S successive ops.gat_forward calls (no save), bit for bit; the maps against the training
    launch's record (save=True: the non-folded form) after the slot -> entity scatter, under the fp64 rule"""
    case = Case(n, B, S, N, d0, d1, device, seed=3)
    got = case.run()
    h = case.d_hidden0
    worst = {}
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    for s in range(S):
        src1 = case.d_src1[:, :, s] if d1 else None
        nz = case.d_noise[:, :, s].contiguous()
        h_prev = h
        h, _ = ops.gat_forward(case.arena, case.d_src0[:, :, s], src1, h_prev, nz)
        _sync(device)
        assert torch.equal(got["latent"][:, :, s].view(torch.int32), h.view(torch.int32)), ("latent bits differ at step", s)
        _, saved = ops.gat_forward(case.arena, case.d_src0[:, :, s], src1, h_prev, nz, save=True)
        _sync(device)
        for k in ("soft", "hard"):
            rec = scatter(saved[k].cpu().reshape(n, B, N, N - 1), N)
            for i in range(n):
                e32 = _grad_err(r32[k][i, :, s], r64[k][i, :, s])
                err = _grad_err(got[k][i, :, s].cpu(), rec[i])
                _worse(worst, k + "_vs_record", err)
                assert err <= _bound(e32), (k, i, s, err, e32)
    return worst


def check_sentinel(device, n, B, S, N, d0=5, d1=8):
    """outputs carved out of sentinel-filled buffers with padded rows: padding, entities >= N and unrequested outputs stay untouched"""
    case = Case(n, B, S, N, d0, d1, device, seed=9)
    ref = case.run()
    shapes = {"latent": (N, A), "soft": (N, N), "hard": (N, N), "attn": (N, N)}

    def carve(k, shift=0.0):
        r, c = shapes[k]
        total = n * B * S * (r + 2) * c + 64
        sent = 0.5 + shift + (torch.arange(total, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        body = buf[32:32 + n * B * S * (r + 2) * c].view(n, B, S, r + 2, c)
        return sent, buf, body[:, :, :, :r]                                     # rows r, r + 1 of every block: entities >= N

    for wanted in (("latent", "soft", "hard", "attn"), ("latent",), ("attn",)):
        bufs = {k: carve(k) for k in shapes}
        got = case.run(want=wanted + ("stats",), out={k: bufs[k][2] for k in wanted})
        assert torch.equal(got["stats"], ref["stats"])
        for k, (sent, buf, view) in bufs.items():
            r, c = shapes[k]
            host = buf.cpu()
            if k not in wanted:
                assert torch.equal(host.view(torch.int32), sent.view(torch.int32)), (k, "was not asked for and was written")
                continue
            assert torch.equal(view, ref[k]), (k, "differs inside a padded buffer")
            mask = torch.ones_like(host, dtype=torch.bool)
            mview = mask[32:32 + n * B * S * (r + 2) * c].view(n, B, S, r + 2, c)
            mview[:, :, :, :r] = False
            assert torch.equal(host[mask].view(torch.int32), sent[mask].view(torch.int32)), (k, "a float outside the owned rows was written")
    # every owned float is written: a second, shifted sentinel ends with the same contents
    b2 = {k: carve(k, 0.25) for k in shapes}
    case.run(want=tuple(shapes), out={k: b2[k][2] for k in shapes})
    for k in shapes:
        assert torch.equal(b2[k][2], ref[k]), (k, "an owned float was left unwritten")
    return {}


def check_optional_operands(device, n=2, B=2, S=3, N=7, d0=5, d1=8):
    """hidden0 null == zeros, weight null == ones, zero weights remove exactly those steps, presence_col < 0 counts all, d1 = 0"""
    case = Case(n, B, S, N, d0, d1, device, seed=5)
    worst = {}
    base = case.run()
    none = case.run(hidden0=False)
    assert_vs_fp64(case, none, worst, "hidden0 null", hidden0=False)
    case.hidden0.zero_()
    case.upload()
    zero = case.run()
    for k in ("latent",) + MAPS + ("stats",):
        assert torch.equal(none[k].view(torch.int32), zero[k].view(torch.int32)), (k, "hidden0 null != explicit zeros")
    unweighted = case.run(weight=False)
    assert_vs_fp64(case, unweighted, worst, "weight null", weight=False)
    case.weight.fill_(1.0)
    case.upload()
    ones = case.run()
    assert torch.equal(unweighted["stats"], ones["stats"])
    case.weight[:, :, 1] = 0.0
    case.upload()
    holes = case.run()
    assert torch.equal(holes["stats"][:, :, 1].cpu(), torch.zeros(n, B, 6))
    assert torch.equal(holes["stats"][:, :, [0, 2]], ones["stats"][:, :, [0, 2]])
    for k in ("latent",) + MAPS:
        assert torch.equal(holes[k], ones[k]), (k, "the weights entered an output other than the sums")
    every = case.run(presence_col=-1, weight=False)
    assert_vs_fp64(case, every, worst, "presence_col -1", presence_col=-1, weight=False)
    assert torch.equal(every["stats"][..., 0].cpu(), torch.full((n, B, S), float(N)))
    assert torch.equal(every["stats"][..., 1].cpu(), torch.full((n, B, S), float(N * (N - 1))))
    del base
    c0 = Case(n, B, S, N, d0, 0, device, seed=6)
    assert_vs_fp64(c0, c0.run(), worst, "d1 = 0")
    return worst


def check_repeatable(device, reps, n=2, B=2, S=3, N=33, d0=5, d1=8):
    """``reps`` launches on the same inputs: identical bits for every output and sum"""
    case = Case(n, B, S, N, d0, d1, device, seed=1)
    first = case.run()
    for _ in range(reps - 1):
        again = case.run()
        for k in ("latent",) + MAPS + ("stats",):
            assert torch.equal(again[k].view(torch.int32), first[k].view(torch.int32)), k
    return {}


def check_bad_arguments(device):
    """each of these is refused with its code and a message, without a launch"""
    case = Case(1, 1, 2, 5, 5, 8, device, seed=2)
    good = case.run()
    lib = ops._lib(None)
    a, _ = ops.gat_trace_args(case.arena, case.d_src0, case.d_src1, case.d_hidden0, case.d_noise, want=("latent",) + MAPS + ("stats",),
                              weight=case.d_weight, presence_col=0, out=good)

    def refused(code, **fields):
        keep = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        rc = lib.c.iplan_gat_trace(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, v in keep.items():
            setattr(a, k, v)
        assert rc == code and "iplan_gat_trace" in msg, (fields, rc, msg)

    EINVAL, EALIGN = _codes()
    refused(EINVAL, N=1)
    refused(EINVAL, N=65)
    refused(EINVAL, S=0)
    refused(EINVAL, latent=None, soft=None, hard=None, attn=None, stats=None)
    refused(EALIGN, latent=good["latent"].data_ptr() + 4)
    again = case.run()
    assert torch.equal(again["latent"], good["latent"])
    return {}


def _codes():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iplan_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"(IPLAN_E\w+)\s*=\s*(-?\d+)", text)}
    return vals["IPLAN_EINVAL"], vals["IPLAN_EALIGN"]


# ------------------------------------------------------------------------------------------------ the methods
def _e2e_args(device, **kw):
    from iplan_amd.config import default_args
    base = dict(use_cuda=torch.device(device).type == "cuda", max_vehicle_num=5, n_agents=2, episode_limit=12, pred_length=3, pred_batch_size=6)
    base.update(kw)
    return default_args("highway", **base)


def _policy_reference(gat, hist, lat, hid0, noise, dtype):
    """hist [E,S,N,d], lat [E,S,N,Z], hid0 [E,N,A], noise [E,S,N,N-1,2] or None of one agent -> latent [E,S,N,A], attn, soft, hard [E,S,N,N]"""
    E, S, N, _ = hist.shape
    p = {k: v.to(dtype) for k, v in gat.items()}
    h = hid0.to(dtype).reshape(E * N, -1)
    out = {k: [] for k in ("latent", "attention", "soft", "hard")}
    for s in range(S):
        nz = (noise[:, s] if noise is not None else torch.zeros(E, N, N - 1, 2)).to(dtype).reshape(-1, 2)
        h, it = O.gat_forward(p, torch.cat([hist[:, s], lat[:, s]], -1).to(dtype), h, nz, return_internals=True)
        soft, hard = scatter(it["soft"], N), scatter(it["hard"], N)
        for k, v in (("latent", h.reshape(E, N, -1)), ("attention", soft * hard), ("soft", soft), ("hard", hard)):
            out[k].append(v)
    return {k: torch.stack(v, 1) for k, v in out.items()}


def check_methods(device, tmp_path, E=3, S=4):
    """attention_map / attention_trace on a loaded checkpoint: numpy and tensor inputs, types, shapes, values against the oracle,
    chunked == unchunked, deferred == inline, deterministic mode draws nothing, nothing of the policy is touched"""
    from iplan_amd import synth
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device)
    pol, gat, _ = _loaded_policy(args, tmp_path, 17)
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    gen = torch.Generator().manual_seed(5)
    hist = synth.make_history(gen, (E, S, nA), N, d, presence_p=0.7)
    lat = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
    hid = torch.randn(E, nA, N, A, generator=gen) * 0.1
    noise = _gumbel(gen, nA, E, S, N, N - 1, 2)
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), opt=[str(o.state_dict()) for o in pol.pred_optimizer])
    worst = {}
    want = ("attention", "soft", "hard")
    res = pol.attention_trace(hist.double().numpy(), lat.numpy(), hidden0=hid.numpy(), noise=noise.to(device), want=want)
    dev_res = pol.attention_trace(hist.to(device), lat.to(device), hidden0=hid.to(device), noise=noise.to(device), want=want,
                                  max_envs_per_launch=1)
    fin = pol.attention_trace(hist.to(device), lat.to(device), hidden0=hid.to(device), noise=noise.to(device), want=want, defer=True)
    assert callable(fin)
    def_res = fin()
    for k, shape in (("latent", (E, S, nA, N, A)),) + tuple((m, (E, S, nA, N, N)) for m in want):
        assert isinstance(res[k], np.ndarray) and res[k].shape == shape, (k, res[k].shape)
        assert torch.is_tensor(dev_res[k]) and dev_res[k].device.type == torch.device(device).type
        assert np.array_equal(dev_res[k].cpu().numpy(), res[k]) and np.array_equal(def_res[k].cpu().numpy(), res[k]), (k, "chunked / deferred differ")
    for k in ("gate", "attention_per_ego", "present_mass", "entropy", "egos", "pairs"):
        assert isinstance(res["stats"][k], np.ndarray) and res["stats"][k].shape == (nA, S)
        assert np.array_equal(res["stats"][k], dev_res["stats"][k], equal_nan=True) and np.array_equal(res["stats"][k], def_res["stats"][k], equal_nan=True), k
    for i in range(nA):
        r64 = _policy_reference(gat[i], hist[:, :, i], lat[:, :, i], hid[:, i], noise[i], torch.float64)
        r32 = _policy_reference(gat[i], hist[:, :, i], lat[:, :, i], hid[:, i], noise[i], torch.float32)
        for k in ("latent",) + want:
            for s in range(S):
                e32, err = _grad_err(r32[k][:, s], r64[k][:, s]), _grad_err(torch.as_tensor(res[k][:, s, i]), r64[k][:, s])
                _worse(worst, "method_" + k, err)
                assert err <= _bound(e32), (k, i, s, err, e32)
        pres = (hist[:, :, i, :, 0] != 0).double()                                # [E, S, N]
        pair = pres[..., :, None] * pres[..., None, :] * (1 - torch.eye(N).double())
        g64 = (pair * r64["hard"]).sum((0, 2, 3)) / pair.sum((0, 2, 3))
        g32 = ((pair * r32["hard"].double()).sum((0, 2, 3)) / pair.sum((0, 2, 3)))
        e32, err = _grad_err(g32, g64), _grad_err(torch.as_tensor(res["stats"]["gate"][i]), g64)
        _worse(worst, "method_gate", err)
        assert err <= _bound(e32), ("gate", i, err, e32)
        assert np.array_equal(res["stats"]["egos"][i], pres.sum((0, 2)).numpy())
    # one step: attention_map, its latent bit-identical to GAT_latent_update's
    m_np = pol.attention_map(hist[:, 0].numpy(), hid.numpy(), lat[:, 0].numpy(), noise=noise[:, :, 0].contiguous().to(device))
    m_dev = pol.attention_map(hist[:, 0].to(device), hid.to(device), lat[:, 0].to(device), noise=noise[:, :, 0].contiguous().to(device))
    upd = pol.GAT_latent_update(hist[:, 0].to(device), hid.to(device), lat[:, 0].to(device), noise=noise[:, :, 0].contiguous().to(device))
    _sync(device)
    assert torch.equal(m_dev["latent"].view(torch.int32), upd.view(torch.int32)), "attention_map's latent != GAT_latent_update's"
    for k, shape in (("attention", (E, nA, N, N)), ("soft", (E, nA, N, N)), ("hard", (E, nA, N, N)), ("latent", (E, nA, N, A))):
        assert isinstance(m_np[k], np.ndarray) and m_np[k].shape == shape and torch.is_tensor(m_dev[k])
        assert np.array_equal(m_np[k], m_dev[k].cpu().numpy()) and np.array_equal(m_np[k], res[k][:, 0]), k
    # deterministic mode: no generator is advanced, two calls agree, the values are the oracle's without noise
    states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None)
    d1 = pol.attention_trace(hist.to(device), lat.to(device), hidden0=hid.to(device), deterministic=True)
    d2 = pol.attention_trace(hist.to(device), lat.to(device), hidden0=hid.to(device), deterministic=True, noise=noise.to(device))
    assert torch.equal(torch.get_rng_state(), states[0])
    if states[1] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), states[1])
    assert torch.equal(d1["latent"], d2["latent"]) and torch.equal(d1["attention"], d2["attention"])
    for i in range(nA):
        r64 = _policy_reference(gat[i], hist[:, :, i], lat[:, :, i], hid[:, i], None, torch.float64)
        r32 = _policy_reference(gat[i], hist[:, :, i], lat[:, :, i], hid[:, i], None, torch.float32)
        for s in range(S):
            e32, err = _grad_err(r32["attention"][:, s], r64["attention"][:, s]), _grad_err(d1["attention"][:, s, i].cpu(), r64["attention"][:, s])
            _worse(worst, "deterministic_attention", err)
            assert err <= _bound(e32), ("deterministic", i, s, err, e32)
    # without injected noise it draws its own
    own = pol.attention_trace(hist.to(device), lat.to(device), hidden0=hid.to(device))
    assert torch.isfinite(own["latent"]).all() and np.isfinite(own["stats"]["entropy"]).all()
    # nothing counts: NaN
    nothing = pol.attention_trace(hist.to(device), lat.to(device), weight=torch.zeros(E, S, nA), deterministic=True)
    assert np.isnan(nothing["stats"]["gate"]).all() and (nothing["stats"]["egos"] == 0).all()
    assert torch.equal(pol.gat_arena.data, before["gat"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"]
    return worst


def check_learn_unaffected_by_trace(device, E=2):
    """learn() with injected sel / noise / keep gives the same loss and parameters whether or not an attention_trace ran before it"""
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
    for with_trace in (False, True):
        torch.manual_seed(31)
        np.random.seed(32)
        pol = Prediction_policy(args, _Log())
        if with_trace:
            D = batch.data
            tr = pol.attention_trace(D["history"][:, 1:], D["behavior_latent"][:, :-1], hidden0=D["attention_latent"][:, 0], deterministic=True,
                                     max_envs_per_launch=1)
            assert torch.isfinite(tr["latent"]).all()
        losses = pol.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), pol.gat_arena.data.clone(), pol.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


def check_replays_rollout(device, E=2, N=7, T=6):
    """attention_trace on a rollout's own fields, with the alignment its docstring gives (history[:, 1:], behavior_latent[:, :-1],
    hidden0 = attention_latent[:, 0]) and the rollout's per-step noise, gives batch["attention_latent"][:, 1:] bit for bit -- against
    the rollout's fused launches, not the standalone GAT launch"""
    from iplan_amd.harness import SyntheticLoop
    args = _e2e_args(device, max_vehicle_num=N, episode_limit=T, batch_size_run=E, max_history_len=3)
    nA = args.n_agents
    loop = SyntheticLoop(args, E, seed=4, device=device)
    gen = torch.Generator().manual_seed(15)
    noise = _gumbel(gen, T + 1, nA, E, N, N - 1, 2).to(device)                  # entry T feeds the episode-initial update
    q_all = -torch.log(torch.rand(T, nA, E, args.n_actions, generator=gen).clamp_min(1e-20)).to(device)
    batch = loop.new_batch()
    with torch.no_grad():
        loop._rollout_body(loop.obs_sets[0], batch, noise=noise, q_all=q_all)
    _sync(device)
    D = batch.data
    assert D["attention_latent"][:, 1:].abs().sum() > 0
    res = loop.prediction.attention_trace(D["history"][:, 1:], D["behavior_latent"][:, :-1], hidden0=D["attention_latent"][:, 0],
                                          noise=noise[:T].permute(1, 2, 0, 3, 4, 5).contiguous())
    _sync(device)
    got, ref = res["latent"], D["attention_latent"][:, 1:T + 1]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.equal(got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)), \
        f"the trace's latents differ from the rollout's by up to {(got - ref).abs().max().item():.3g}"
    return {}
