"""TEST INFRASTRUCTURE: neighbour knock-out attribution (csrc/gat_knockout.hip, ops.gat_knockout, Prediction_policy.attention_knockout)
on whatever library is active -- the host emulator in tests/test_emu_knockout.py, the gfx950 build in tests/test_gpu_knockout.py.

The reference of the bit-for-bit checks is the existing path on an EXPLICIT copy of the inputs with the knocked row replaced:
ops.gat_forward (the rollout's launch) for the latents, ops.gat_trace / attention_map for the attention map, ops.predict / predict() for
the forecasts, and plain fp32 torch loops for the two distances.  Ground truth of the values: oracle.gat_forward in fp64 on the same
modified inputs; error = max|got - ref64| / max|ref64| per (net, job) tensor, bound 1e-5 at tau = 1 and 0.25 and max(1e-5, E32_FACTOR x
the fp32 oracle's own error on the same tensor) at tau = 0.01 (tests/oracle_checks.py; N = 2 at tau = 0.01 is not compared: one gate
carries everything there).  The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.attention_checks import _codes, _e2e_args, _gumbel, _sync, _worse
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5
A = 32
# (n_nets, B, N, d0, d1): N at the edges of the 16-row tiles and at the limit; 1 and 5 nets; 1 and 2 scenes; with and without source 1
KERNEL_CASES = [(1, 1, 2, 5, 0), (5, 2, 5, 5, 3), (1, 2, 16, 7, 9), (1, 1, 17, 5, 3), (1, 2, 33, 5, 0), (1, 1, 64, 7, 9)]
# ... each at tau = 1, 0.25 and 0.01, but for N = 2 at 0.01 (one gate carries everything there: the data-derived bound is undefined)
FP64_CASES = [c + (tau,) for c in KERNEL_CASES for tau in (1.0, 0.25, 0.01) if not (c[2] == 2 and tau == 0.01)]
OUTPUTS = ("latent_ko", "attn_ko", "shift_sq")


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(bits(x), bits(y))


def job_list(N):
    """-1 (nothing knocked) and entities at the tile edges: everything up to N = 5, the edges of the 16-row tiles up to 17, the first
    and last entity and the first of the last tile beyond (every job costs a scene and its references)"""
    if N <= 5:
        return [-1] + list(range(N))
    if N <= 17:
        return [-1] + sorted({0, 1, 15, 16, N - 1} & set(range(N)))
    return [-1, 0, 16 * ((N - 1) // 16), N - 1]


class Case:
    """random GAT parameters; src0 / src1 / hidden / base are strided views [n, B, N, .] of env-major buffers [B, n, N * w + pad] whose
    surroundings (the pad floats in front of and behind every scene) are NaN: whatever reads outside its rows poisons its result"""

    def __init__(self, n, B, N, d0, d1, device, seed=0, presence_p=0.8):
        from iplan_amd.arena import ParamArena
        from iplan_amd.config import default_args
        from iplan_amd.nova.GAT_Net import GAT_Net
        self.dims = (n, B, N, d0, d1)
        self.device = device
        torch.manual_seed(11 + 1000 * n + 100 * B + N + 10 * d0 + d1 + seed)
        args = default_args("highway", use_cuda=False)
        self.mods = [GAT_Net(d0 + d1, args) for _ in range(n)]
        self.params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.mods]
        self.arena = ParamArena(self.mods, device)
        gen = torch.Generator().manual_seed(seed + 7 * n + 3 * B + N)
        self.src0 = torch.rand(n, B, N, d0, generator=gen) * 2 - 1
        self.src0[..., 0] = (torch.rand(n, B, N, generator=gen) < presence_p).float()
        self.src1 = torch.softmax(torch.randn(n, B, N, d1, generator=gen), -1) * 4 if d1 else None
        self.hidden = torch.randn(n, B, N, A, generator=gen) * 0.1
        self.noise = _gumbel(gen, n, B, N, N - 1, 2)
        self.base0 = torch.rand(d0, generator=gen) - 0.5
        self.base1 = torch.softmax(torch.randn(d1, generator=gen), -1) if d1 else None
        self.upload()

    def _padded(self, t, front, back):
        """t [n, B, N, w] -> (buffer [B, n, front + N w + back] with NaN pads, the view [n, B, N, w] into it) on the device"""
        n, B, N, w = t.shape
        buf = torch.full((B, n, front + N * w + back), float("nan"))
        buf[:, :, front:front + N * w] = t.permute(1, 0, 2, 3).reshape(B, n, N * w)
        buf = buf.to(self.device)
        return buf, buf[:, :, front:front + N * w].unflatten(-1, (N, w)).permute(1, 0, 2, 3)

    def upload(self):
        dev = self.device
        self.buf0, self.d_src0 = self._padded(self.src0, 3, 2)
        self.buf1, self.d_src1 = self._padded(self.src1, 1, 4) if self.src1 is not None else (None, None)
        self.bufh, self.d_hidden = self._padded(self.hidden, 4, 4)               # (16-byte aligned rows, strides % 4 == 0)
        assert self.d_src0.untyped_storage().nbytes() > 4 * self.d_src0.numel()    # views into larger buffers, not packed copies
        self.d_noise = self.noise.to(dev)
        self.d_base0 = self.base0.to(dev)
        self.d_base1 = self.base1.to(dev) if self.base1 is not None else None

    def knock(self, knock=None):
        return (True, self.dims[4] > 0) if knock is None else knock

    def baseline(self, use):
        return (self.d_base0, self.d_base1) if use else (None, None)

    def base_latent(self, noise=True, tau=0.01, hidden=True):
        """the scene with nothing knocked through the rollout's launch, into a NaN-padded strided buffer -> view [n, B, N, A]"""
        n, B, N = self.dims[:3]
        self.buf_base, view = self._padded(torch.zeros(n, B, N, A), 8, 4)
        ops.gat_forward(self.arena, self.d_src0, self.d_src1, self.d_hidden if hidden else torch.zeros(n, B, N, A, device=self.device),
                        self.d_noise if noise else torch.zeros_like(self.d_noise), tau=tau, out=view)
        _sync(self.device)
        return view

    def run(self, jobs, want=OUTPUTS, noise=True, tau=0.01, knock=None, baseline=False, hidden=True, base=None, out=None):
        if base is None and "shift_sq" in want:
            base = self.base_latent(noise, tau, hidden)
        res = ops.gat_knockout(self.arena, self.d_src0, self.d_src1, self.d_hidden if hidden else None, jobs, base=base,
                               noise=self.d_noise if noise else None, tau=tau, knock=self.knock(knock), baseline=self.baseline(baseline),
                               want=want, out=out)
        _sync(self.device)
        res["base"] = base
        return res

    def modified(self, j, knock=None, baseline=False, device=None):
        """explicit copies (src0, src1) with entity j's row replaced in the knocked sources; j = -1: plain copies"""
        k0, k1 = self.knock(knock)
        s0 = self.src0.clone()
        s1 = self.src1.clone() if self.src1 is not None else None
        if j >= 0:
            if k0:
                s0[:, :, j] = self.base0 if baseline else 0.0
            if k1:
                s1[:, :, j] = self.base1 if baseline else 0.0
        if device is not None:
            s0 = s0.to(device)
            s1 = s1.to(device) if s1 is not None else None
        return s0, s1

    def oracle(self, j, dtype, noise=True, tau=0.01, knock=None, baseline=False):
        """latent [n, B, N, A] of the modified inputs in ``dtype``"""
        n, B, N = self.dims[:3]
        s0, s1 = self.modified(j, knock, baseline)
        out = []
        for i in range(n):
            p = {k: v.to(dtype) for k, v in self.params[i].items()}
            obs = s0[i] if s1 is None else torch.cat([s0[i], s1[i]], -1)
            nz = (self.noise[i] if noise else torch.zeros(B, N, N - 1, 2)).to(dtype).reshape(-1, 2)
            out.append(O.gat_forward(p, obs.to(dtype), self.hidden[i].to(dtype).reshape(B * N, A), nz, tau=tau).reshape(B, N, A))
        return torch.stack(out)


def host_shift_sq(ko, base):
    """sum_c (ko - base)^2 over the last dim, c ascending, every product and every add a rounded fp32 operation of its own"""
    ko, base = ko.cpu(), base.cpu()
    s = torch.zeros(ko.shape[:-1], dtype=torch.float32)
    for c in range(ko.shape[-1]):
        d = ko[..., c] - base[..., c]
        s = s + d * d
    return s


# ------------------------------------------------------------------------------------------------ 1 + 3: the existing path's bits
def check_same_bits(device, n, B, N, d0, d1, noise=True, knock=None, baseline=False, tau=0.01):
    """latent_ko[j] == ops.gat_forward on the modified copy, job -1 == the base latent, attn_ko[j] == the trace launch's map on the
    modified copy, shift_sq == the fp32 host loop -- all bit for bit"""
    case = Case(n, B, N, d0, d1, device, seed=1)
    jobs = job_list(N)
    got = case.run(jobs, noise=noise, knock=knock, baseline=baseline, tau=tau)
    base = got["base"]
    nz = case.d_noise if noise else torch.zeros_like(case.d_noise)
    moved = 0
    for slot, j in enumerate(jobs):
        s0, s1 = case.modified(j, knock, baseline, device)
        ref, _ = ops.gat_forward(case.arena, s0, s1, case.d_hidden, nz, tau=tau)
        tr = ops.gat_trace(case.arena, s0.unsqueeze(2), None if s1 is None else s1.unsqueeze(2), case.d_hidden, nz.unsqueeze(2) if noise else None,
                           tau=tau, want=("attn",))
        _sync(device)
        assert same_bits(got["latent_ko"][:, :, slot], ref), ("latent_ko differs from gat_forward on the modified copy", j)
        assert same_bits(got["attn_ko"][:, :, slot], tr["attn"][:, :, 0]), ("attn_ko differs from the trace's map on the modified copy", j)
        if j < 0:
            assert same_bits(got["latent_ko"][:, :, slot], base), "job -1 differs from the base latent"
        else:
            moved += int(not same_bits(ref, base))
    assert moved > 0, "no knocked latent differs from the base: the comparison says nothing"
    host = host_shift_sq(got["latent_ko"], base.unsqueeze(2).expand_as(got["latent_ko"]))
    assert same_bits(got["shift_sq"].cpu(), host), "shift_sq differs from the fp32 host loop"
    assert torch.isfinite(got["latent_ko"]).all() and torch.isfinite(got["shift_sq"]).all() and torch.isfinite(got["attn_ko"]).all()
    return {"shift_sq_max": float(got["shift_sq"].max())}


# ------------------------------------------------------------------------------------------------ 2: exact zeros
def check_exact_zeros(device, n, B, N, d0, d1, baseline):
    """rows that already equal the baseline in the knocked sources: latent_ko == latent bit for bit, shift_sq exactly 0.0"""
    case = Case(n, B, N, d0, d1, device, seed=2)
    quiet = sorted({0, N // 2, N - 1})
    for j in quiet:
        case.src0[:, :, j] = case.base0 if baseline else 0.0
        if d1:
            case.src1[:, :, j] = case.base1 if baseline else 0.0
    case.upload()
    loud = [j for j in range(N) if j not in quiet][:1]
    for noise in (True, False):
        got = case.run(quiet + loud, noise=noise, baseline=baseline)
        for slot in range(len(quiet)):
            assert same_bits(got["latent_ko"][:, :, slot], got["base"]), ("a row equal to its baseline moved the latent", quiet[slot])
            assert torch.equal(bits(got["shift_sq"][:, :, slot]), torch.zeros_like(bits(got["shift_sq"][:, :, slot]))), "shift_sq is not +0.0"
        if loud:
            assert (got["shift_sq"][:, :, len(quiet)] > 0).any(), "an informative row moved nothing"
    return {}


# ------------------------------------------------------------------------------------------------ 4: against fp64
def check_vs_fp64(device, n, B, N, d0, d1, tau):
    assert not (N == 2 and tau == 0.01)
    case = Case(n, B, N, d0, d1, device, seed=3)
    jobs = [j for j in job_list(N) if j >= 0][:4]
    worst = {}
    for noise in (True, False):
        got = case.run(jobs, want=("latent_ko",), noise=noise, tau=tau)["latent_ko"].cpu()
        b64 = case.oracle(-1, torch.float64, noise, tau)
        for slot, j in enumerate(jobs):
            r64 = case.oracle(j, torch.float64, noise, tau)
            assert (r64 - b64).abs().max() > 0, ("the oracle's knocked latent equals its base", j)
            r32 = case.oracle(j, torch.float32, noise, tau) if tau == 0.01 else None
            for i in range(n):
                err = _grad_err(got[i, :, slot], r64[i])
                e32 = _grad_err(r32[i], r64[i]) if r32 is not None else 0.0
                bound = max(TOL, E32_FACTOR * e32) if tau == 0.01 else TOL
                print("knockout", (n, B, N, d0, d1), "tau", tau, "noise", noise, "job", j, "net", i, "err", err, "e32", e32)
                _worse(worst, f"latent_ko_tau{tau}", err)
                _worse(worst, f"e32_tau{tau}", e32)
                assert err <= bound, (tau, noise, j, i, err, e32)
    return worst


# ------------------------------------------------------------------------------------------------ 5: independence (the kernel)
def check_independence(device, n=2, B=2, N=7, d0=5, d1=3):
    """a slot's bits do not change with the order or length of the job list, duplicates, the other scenes, or the outputs asked for"""
    case = Case(n, B, N, d0, d1, device, seed=4)
    jobs = [3, -1, N - 1, 0]
    ref = case.run(jobs)
    base = ref["base"]
    by_job = {j: {k: ref[k][:, :, s] for k in OUTPUTS} for s, j in enumerate(jobs)}

    def agree(got, lst, what, scenes=slice(None)):
        for s, j in enumerate(lst):
            for k in OUTPUTS:
                if k in got:
                    assert same_bits(got[k][:, :, s], by_job[j][k][:, scenes]), (what, k, j)
    agree(case.run(jobs[::-1], base=base), jobs[::-1], "reversed list")
    agree(case.run([N - 1], base=base), [N - 1], "one job")
    agree(case.run([0, 0, 3, 0, -1, -1], base=base), [0, 0, 3, 0, -1, -1], "duplicates")
    for want in (("latent_ko",), ("attn_ko",), ("shift_sq",), ("shift_sq", "attn_ko")):
        agree(case.run(jobs, want=want, base=base), jobs, want)
    # the other scenes of the launch: one scene alone
    got = ops.gat_knockout(case.arena, case.d_src0[:, 1:], case.d_src1[:, 1:], case.d_hidden[:, 1:], jobs, base=base[:, 1:],
                           noise=case.d_noise[:, 1:].contiguous(), want=OUTPUTS)
    _sync(device)
    agree(got, jobs, "one scene alone", slice(1, 2))
    return {}


def check_repeatable(device, reps, n=1, B=2, N=17, d0=5, d1=3):
    case = Case(n, B, N, d0, d1, device, seed=5)
    jobs = job_list(N)
    first = case.run(jobs)
    for _ in range(reps - 1):
        again = case.run(jobs, base=first["base"])
        for k in OUTPUTS:
            assert same_bits(again[k], first[k]), k
    return {}


# ------------------------------------------------------------------------------------------------ 6: ownership
def check_ownership(device, n, B, N, d0=5, d1=3):
    """outputs as strided views inside sentinel-filled buffers (padded rows, padded job slots), inputs inside NaN pads (Case): only the
    owned floats change, every owned float is written, an output not asked for is not written"""
    case = Case(n, B, N, d0, d1, device, seed=6)
    jobs = job_list(N)[:4]
    J = len(jobs)
    ref = case.run(jobs)
    base_buf = case.buf_base                                                       # (the buffer ref["base"] is a view of)
    base_before = base_buf.cpu().clone()
    shapes = {"latent_ko": (N, A), "attn_ko": (N, N), "shift_sq": (1, N)}

    def carve(k, shift=0.0):
        """a slot's [r, c] block is packed (the kernel's layout); the slot is padded behind it (a multiple of 4 floats: the latent's
        strides), one job slot more than J follows every scene, 32 guard floats at either end"""
        r, c = shapes[k]
        slot = r * c + (-(r * c)) % 4 + 8
        body_len = n * B * (J + 1) * slot
        sent = 0.5 + shift + (torch.arange(body_len + 64, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        view = buf[32:32 + body_len].view(n, B, J + 1, slot)[:, :, :J, :r * c].unflatten(-1, (r, c))
        if k == "shift_sq":
            view = view[:, :, :, 0]
        own = torch.zeros(body_len + 64, dtype=torch.bool)
        own[32:32 + body_len].view(n, B, J + 1, slot)[:, :, :J, :r * c] = True
        return sent, buf, view, own

    for wanted in (OUTPUTS, ("shift_sq",), ("latent_ko", "attn_ko")):
        bufs = {k: carve(k) for k in shapes}
        case.run(jobs, want=wanted, base=ref["base"], out={k: bufs[k][2] for k in wanted})
        for k, (sent, buf, view, own) in bufs.items():
            host = buf.cpu()
            if k not in wanted:
                assert torch.equal(bits(host), bits(sent)), (k, "was not asked for and was written")
                continue
            assert same_bits(view, ref[k]), (k, "differs inside a padded buffer")
            assert torch.equal(bits(host[~own]), bits(sent[~own])), (k, "a float outside the owned elements was written")
    b2 = {k: carve(k, 0.25) for k in shapes}
    case.run(jobs, base=ref["base"], out={k: b2[k][2] for k in shapes})
    for k in shapes:
        assert same_bits(b2[k][2], ref[k]), (k, "an owned float was left unwritten")
    # every input the kernel reads, and its NaN surroundings, is as it was (the base latent: as the launch in front left it)
    n_, B_, N_ = case.dims[:3]
    for buf, t, front in ((case.buf0, case.src0, 3), (case.buf1, case.src1, 1), (case.bufh, case.hidden, 4), (base_buf, ref["base"].cpu(), 8)):
        w = t.shape[2] * t.shape[3]
        host = buf.cpu()
        assert torch.isnan(host[:, :, :front]).all() and torch.isnan(host[:, :, front + w:]).all()
        assert same_bits(host[:, :, front:front + w], t.permute(1, 0, 2, 3).reshape(B_, n_, w))
    assert same_bits(base_buf.cpu(), base_before), "the base latent's buffer was written"
    assert same_bits(case.d_noise.cpu(), case.noise) and same_bits(case.d_base0.cpu(), case.base0)
    return {}


# ------------------------------------------------------------------------------------------------ 9: refusals (entry point and op)
def check_bad_arguments(device):
    """each of these is refused with its code and a message, without a launch; the op refuses on the host"""
    case = Case(1, 2, 5, 5, 3, device, seed=7)
    jobs = [-1, 0, 4]
    good = case.run(jobs)
    lib = ops._lib(None)
    a, _, keep = ops.gat_knockout_args(case.arena, case.d_src0, case.d_src1, case.d_hidden, jobs, base=good["base"], noise=case.d_noise,
                                       want=OUTPUTS, out={k: good[k] for k in OUTPUTS})
    EINVAL, EALIGN = _codes()

    def refused(code, **fields):
        saved = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        rc = lib.c.iplan_gat_knockout(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, v in saved.items():
            setattr(a, k, v)
        assert rc == code and "iplan_gat_knockout" in msg, (fields, rc, msg)

    def host_jobs(*v):
        arr = (L.C.c_int32 * len(v))(*v)
        keep.append(arr)
        return L.C.cast(arr, L.C.c_void_p)

    rc = lib.c.iplan_gat_knockout(None, L.C.c_void_p(0))
    assert rc == EINVAL
    refused(EINVAL, N=1)
    refused(EINVAL, N=65)
    refused(EINVAL, J=0)
    refused(EINVAL, J=-3)
    refused(EINVAL, jobs_host=host_jobs(-1, 0, 5))
    refused(EINVAL, jobs_host=host_jobs(-2, 0, 4))
    refused(EINVAL, jobs_host=None)
    refused(EINVAL, jobs=None)
    refused(EINVAL, d1=0, knock1=1)
    refused(EINVAL, src0=None)
    refused(EINVAL, src1=None)
    refused(EINVAL, params=None)
    refused(EINVAL, latent_ko=None, attn_ko=None, shift_sq=None)
    refused(EINVAL, base=None)
    refused(EINVAL, n_nets=1 << 15, B=1 << 15, J=4)                              # 2^32 workgroups
    refused(EALIGN, latent_ko=good["latent_ko"].data_ptr() + 4)
    refused(EALIGN, lat_s_job=a.lat_s_job + 1)
    refused(EALIGN, hidden=case.d_hidden.data_ptr() + 4)
    refused(EALIGN, h_s_b=a.h_s_b + 2)
    lib.call("iplan_gat_knockout", a, L.current_stream(device))                    # the descriptor itself is good
    _sync(device)
    again = case.run(jobs, base=good["base"])
    for k in OUTPUTS:
        assert same_bits(again[k], good[k]), k

    def op_refuses(**kw):
        args = dict(jobs=jobs, base=good["base"], want=OUTPUTS)
        args.update(kw)
        j = args.pop("jobs")
        try:
            ops.gat_knockout(case.arena, case.d_src0, args.pop("src1", case.d_src1), case.d_hidden, j, noise=case.d_noise, **args)
        except AssertionError:
            return
        raise AssertionError(f"ops.gat_knockout accepted {kw}")
    op_refuses(jobs=[])
    op_refuses(jobs=[5])
    op_refuses(jobs=[-2])
    op_refuses(want=())
    op_refuses(want=("latent",))
    op_refuses(base=None)
    op_refuses(src1=None, knock=(True, True))
    op_refuses(baseline=(case.d_base0[:3], None))
    op_refuses(out={"latent_ko": torch.empty(1, 2, 3, 5, A, device=device)[:, :, :, :, :16]})
    op_refuses(out={"shift_sq": torch.empty(1, 2, 4, 5, device=device)})       # a job slot too many
    return {}


# ------------------------------------------------------------------------------------------------ the method
def _method_inputs(args, E, S, seed, device):
    from iplan_amd import synth
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    gen = torch.Generator().manual_seed(seed)
    hist = synth.make_history(gen, (E, S, nA), N, d, presence_p=0.7)
    lat = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
    hid = torch.randn(E, S, nA, N, A, generator=gen) * 0.1
    noise = _gumbel(gen, nA, E, S, N, N - 1, 2)
    return hist, lat, hid, noise


def _host_forecast_shift(pk, pb, pos):
    """pk [.., J, N, P, d], pb [.., N, P, d] -> [.., J, N, P]: squared differences of the pos columns added in order, then sqrt"""
    acc = None
    for c in pos:
        diff = pk[..., c] - pb.unsqueeze(-4)[..., c]
        acc = diff * diff if acc is None else acc + diff * diff
    return acc.sqrt()


def check_methods(device, tmp_path, E, S, N=5):
    """10 + 7 + 5 (chunking) + 1 at the method: attention_knockout on a loaded checkpoint -- numpy and device round trips, every result
    against the existing methods on explicit copies, the forecast chain, chunked == unchunked, the sources and baselines, summary"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device, max_vehicle_num=N)
    pol, gat, _ = _loaded_policy(args, tmp_path, 23)
    nA, d, Z, P = args.n_agents, args.obs_shape_single, args.latent_dim, args.pred_length
    hist, lat, hid, noise = _method_inputs(args, E, S, 8, device)
    hist[0, 0, :, 1] = 0.0                                                         # an unseen vehicle: knocking it changes nothing
    lat[0, 0, :, 1] = 0.0
    dv = lambda t: t.to(device)                                                    # noqa: E731
    worst = {}
    want = ("shift", "latent_ko", "attention_ko")
    r_np = pol.attention_knockout(hist.double().numpy(), lat.numpy(), hid.numpy(), noise=noise.numpy(), deterministic=False, want=want, forecast=True)
    r_dev = pol.attention_knockout(dv(hist), dv(lat), dv(hid), noise=dv(noise), deterministic=False, want=want, forecast=True)
    per_row = 4 * nA * (2 * N * (N - 1) + N * A + N * P * d)
    per_job = 4 * nA * (N + N * A + N * N + N * P * (d + 1))
    tiny = (per_row + 2 * per_job + 8) / (1 << 20)                                # one row and two of the five jobs per chunk
    assert E * S >= 2                                                              # (so the tiny workspace splits the rows too)
    r_chunk = pol.attention_knockout(dv(hist), dv(lat), dv(hid), noise=dv(noise), deterministic=False, want=want, forecast=True,
                                     max_workspace_mb=tiny)
    _sync(device)
    shapes = {"latent": (E, S, nA, N, A), "latent_shift": (E, S, nA, N, N), "latent_ko": (E, S, nA, N, N, A), "attention_ko": (E, S, nA, N, N, N),
              "pred": (E, S, nA, N, P, d), "forecast_shift": (E, S, nA, N, N, P)}
    for k, shape in shapes.items():
        assert isinstance(r_np[k], np.ndarray) and r_np[k].shape == shape and r_np[k].dtype == np.float32, (k, r_np[k].shape)
        assert torch.is_tensor(r_dev[k]) and r_dev[k].device.type == torch.device(device).type and r_dev[k].shape == shape, k
        assert np.array_equal(r_dev[k].cpu().numpy().view(np.int32), r_np[k].view(np.int32)), (k, "numpy and device round trips differ")
        assert same_bits(r_chunk[k], r_dev[k]), (k, "chunked and unchunked calls differ")
    for r in (r_np, r_dev, r_chunk):
        assert np.array_equal(r["knocked"], np.arange(N)) and r["summary"].shape == (nA, 2) and r["summary"].dtype == np.float64
        assert np.array_equal(r["summary"], r_np["summary"], equal_nan=True)
    # against the existing methods, step by step, on explicit copies
    for s in range(S):
        nz = dv(noise[:, :, s].contiguous())
        upd = pol.GAT_latent_update(dv(hist[:, s]), dv(hid[:, s]), dv(lat[:, s]), noise=nz)
        prd = pol.predict(dv(hist[:, s]), dv(hid[:, s]), dv(lat[:, s]), noise=nz)
        _sync(device)
        assert same_bits(r_dev["latent"][:, s], upd), "latent != GAT_latent_update's"
        assert same_bits(r_dev["pred"][:, s], prd), "pred != predict()'s"
        for j in range(N):
            h2, l2 = hist[:, s].clone(), lat[:, s].clone()
            h2[:, :, j] = 0.0
            l2[:, :, j] = 0.0
            ko = pol.GAT_latent_update(dv(h2), dv(hid[:, s]), dv(l2), noise=nz)
            am = pol.attention_map(dv(h2), dv(hid[:, s]), dv(l2), noise=nz)["attention"]
            _sync(device)
            assert same_bits(r_dev["latent_ko"][:, s, :, j], ko), ("latent_ko != GAT_latent_update on the modified copy", s, j)
            assert same_bits(r_dev["attention_ko"][:, s, :, j], am), ("attention_ko != attention_map on the modified copy", s, j)
    # latent_shift: torch's sqrt of the fp32 host loop; forecast_shift: the host computation from ops.predict on latent_ko
    ko, base = r_dev["latent_ko"].cpu(), r_dev["latent"].cpu()
    sq = host_shift_sq(ko, base.unsqueeze(3).expand_as(ko))                        # [E, S, nA, J, N]
    # (torch's sqrt on the device the method ran on: the distance is promised as torch's sqrt of the kernel's sum of squares)
    assert same_bits(r_dev["latent_shift"].cpu(), sq.to(device).sqrt().cpu().transpose(3, 4)), "latent_shift != torch's sqrt of the host loop"
    h_dev = dv(hist).contiguous()
    for s in range(S):
        hs = h_dev[:, s].contiguous()                                              # [E, nA, N, d]
        off = pol._start_offsets(hs)
        offj = off[:, :, None].expand(nA, E, N).reshape(nA, E * N).contiguous()
        h0 = r_dev["latent_ko"][:, s].permute(1, 0, 2, 3, 4).contiguous().view(nA, E * N * N, A)
        pk = ops.predict(pol.dec_arena, hs, offj, hs.stride(2), 0, h0, N, P, d, checked=True)["pred"].view(nA, E, N, N, P, d)
        fs = _host_forecast_shift(pk, r_dev["pred"][:, s].permute(1, 0, 2, 3, 4), (1, 2))      # [nA, E, J, N, P]
        _sync(device)
        assert same_bits(r_dev["forecast_shift"][:, s], fs.permute(1, 0, 3, 2, 4)), ("forecast_shift != the host computation", s)
    same = (bits(ko) == bits(base.unsqueeze(3).expand_as(ko))).all(-1).transpose(3, 4)      # [E, S, nA, N(ego), J]: latent_ko[j][i] == latent[i]
    assert same[0, 0, :, :, 1].all(), "knocking the unseen vehicle moved a latent"
    assert (r_dev["forecast_shift"].cpu()[same] == 0).all() and (r_dev["latent_shift"].cpu()[same] == 0).all()
    assert (r_dev["latent_shift"] > 0).any() and (r_dev["forecast_shift"] > 0).any()
    # summary against its definition
    pres = hist[..., 0] != 0                                                       # [E, S, nA, N]
    shift = r_np["latent_shift"].astype(np.float64)
    for i in range(nA):
        p = pres[:, :, i].numpy()
        pair = p[:, :, :, None] & p[:, :, None, :]
        eye = np.eye(N, dtype=bool)[None, None]
        for col, m in enumerate((pair & ~eye, pair & eye)):
            ref = shift[:, :, i][m].mean() if m.any() else np.nan
            assert np.isclose(r_np["summary"][i, col], ref, rtol=1e-12, equal_nan=True), (i, col, r_np["summary"][i, col], ref)
    every = pol.attention_knockout(dv(hist), dv(lat), dv(hid), presence_col=-1)
    assert np.allclose(every["summary"][:, 0], [shift_all(every, i, N, False) for i in range(nA)], rtol=1e-12)
    assert np.allclose(every["summary"][:, 1], [shift_all(every, i, N, True) for i in range(nA)], rtol=1e-12)
    # the sources, a baseline, a subset of entities with a duplicate, hidden = None, tau
    base_rows = (torch.rand(d) - 0.5, torch.softmax(torch.randn(Z), -1))
    ents = [3, 0, 3]
    h1, l1, B1 = hist[:1], lat[:1], S                                             # (one environment: every variant is a launch chain of its own)
    rows = lambda t: dv(t).permute(2, 0, 1, 3, 4).reshape(nA, B1, N, t.shape[-1])  # noqa: E731
    for sources, baseline in ((("behavior",), None), (("history",), None), (("history", "behavior"), base_rows), ("behavior", (None, base_rows[1]))):
        r = pol.attention_knockout(dv(h1), dv(l1), None, entities=ents, sources=sources, baseline=baseline, want=("shift", "latent_ko"), tau=0.25)
        assert r["latent_shift"].shape == (1, S, nA, N, 3) and np.array_equal(r["knocked"], ents)
        src = (sources,) if isinstance(sources, str) else sources
        for slot, j in enumerate(ents[:2]):
            h2, l2 = h1.clone(), l1.clone()
            if "history" in src:
                h2[..., j, :] = 0.0 if baseline is None or baseline[0] is None else baseline[0]
            if "behavior" in src:
                l2[..., j, :] = 0.0 if baseline is None or baseline[1] is None else baseline[1]
            refl, _ = ops.gat_forward(pol.gat_arena, rows(h2), rows(l2), torch.zeros(nA, B1, N, A, device=device),
                                      torch.zeros(nA, B1, N, N - 1, 2, device=device), tau=0.25)
            _sync(device)
            got = r["latent_ko"][:, :, :, slot].permute(2, 0, 1, 3, 4).reshape(nA, B1, N, A)
            assert same_bits(got, refl), (sources, "latent_ko differs from gat_forward on the modified copy", j)
        assert same_bits(r["latent_ko"][:, :, :, 0], r["latent_ko"][:, :, :, 2]), "a duplicate entity gave other bits"
    # ``want`` is honoured: without "shift" no distance and no summary, and the other results keep their bits
    only = pol.attention_knockout(dv(hist), dv(lat), dv(hid), noise=dv(noise), deterministic=False, want=("latent_ko",))
    assert set(only) == {"latent", "latent_ko", "knocked"}, sorted(only)
    assert same_bits(only["latent_ko"], r_dev["latent_ko"]) and same_bits(only["latent"], r_dev["latent"])
    fonly = pol.attention_knockout(dv(hist), dv(lat), dv(hid), noise=dv(noise), deterministic=False, want=(), forecast=True)
    assert set(fonly) == {"latent", "pred", "forecast_shift", "knocked"}, sorted(fonly)
    assert same_bits(fonly["forecast_shift"], r_dev["forecast_shift"]) and same_bits(fonly["pred"], r_dev["pred"])
    worst["latent_shift_max"] = float(shift.max())
    worst["forecast_shift_max"] = float(r_np["forecast_shift"].max())
    return worst


def shift_all(res, i, N, diag):
    s = res["latent_shift"][:, :, i].double().cpu().numpy()
    eye = np.eye(N, dtype=bool)
    return s[..., eye].mean() if diag else s[..., ~eye].mean()


def check_nothing_touched(device, tmp_path, reps):
    """the call touches no parameter, gradient entry, optimiser state; in the deterministic mode no generator; ``reps`` calls agree"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device)
    pol, _, _ = _loaded_policy(args, tmp_path, 29)
    hist, lat, hid, noise = _method_inputs(args, 2, 2, 9, device)
    dv = lambda t: t.to(device)                                                    # noqa: E731
    pol.gat_arena.grad.normal_()
    pol.dec_arena.grad.normal_()
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), ggat=pol.gat_arena.grad.clone(), gdec=pol.dec_arena.grad.clone(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer])
    states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, np.random.get_state()[1].copy())
    inputs = [dv(hist), dv(lat), dv(hid)]
    copies = [t.clone() for t in inputs]
    first = pol.attention_knockout(*inputs, want=("shift", "latent_ko", "attention_ko"), forecast=True)
    for _ in range(reps - 1):
        again = pol.attention_knockout(*inputs, want=("shift", "latent_ko", "attention_ko"), forecast=True)
        for k, v in first.items():
            if torch.is_tensor(v):
                assert same_bits(again[k], v), k
        assert np.array_equal(again["summary"], first["summary"], equal_nan=True)
    assert torch.equal(torch.get_rng_state(), states[0]) and np.array_equal(np.random.get_state()[1], states[2])
    if states[1] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), states[1])
    for t, c in zip(inputs, copies):
        assert same_bits(t, c), "an input was written"
    assert same_bits(pol.gat_arena.data, before["gat"]) and same_bits(pol.dec_arena.data, before["dec"])
    assert same_bits(pol.gat_arena.grad, before["ggat"]) and same_bits(pol.dec_arena.grad, before["gdec"])
    assert [str(o.state_dict()) for o in pol.pred_optimizer] == before["opt"]
    # outside the deterministic mode it draws its own noise when none is given
    own = pol.attention_knockout(*inputs, deterministic=False)
    assert torch.isfinite(own["latent_shift"]).all()
    return {}


def check_learn_unaffected(device, E=2):
    """learn() with injected sel / noise / keep gives the same loss and parameters whether or not an attention_knockout ran before it"""
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
            r = pol.attention_knockout(D["history"][:, 1:4], D["behavior_latent"][:, :3], D["attention_latent"][:, :3], forecast=True)
            assert torch.isfinite(r["latent_shift"]).all() and torch.isfinite(r["forecast_shift"]).all()
        losses = pol.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), pol.gat_arena.data.clone(), pol.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


def check_method_refusals(device):
    """every refusal of attention_knockout raises ValueError before anything is launched"""
    from iplan_amd.nova.prediction_policy import Prediction_policy
    args = _e2e_args(device)
    pol = Prediction_policy(args, _Log())
    E, S = 1, 2
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    hist, lat, hid, noise = _method_inputs(args, E, S, 10, device)

    def refuses(*a, **kw):
        try:
            pol.attention_knockout(*a, **kw)
        except ValueError:
            return
        raise AssertionError(f"attention_knockout accepted {kw}")
    refuses(hist[:, 0], lat, hid)
    refuses(hist[:, :, :1], lat, hid)
    refuses(hist[..., :3], lat, hid)
    refuses(hist, None, hid)
    refuses(hist, lat[:, :1], hid)
    refuses(hist, lat, hid[..., :16])
    refuses(hist, lat, hid, entities=[])
    refuses(hist, lat, hid, entities=[N])
    refuses(hist, lat, hid, entities=[-1])
    refuses(hist, lat, hid, entities=[0.5])
    refuses(hist, lat, hid, entities=3)
    refuses(hist, lat, hid, sources=())
    refuses(hist, lat, hid, sources=("history", "intent"))
    refuses(hist, lat, hid, baseline=(torch.zeros(d + 1), None))
    refuses(hist, lat, hid, baseline=(None, torch.zeros(Z - 1)))
    refuses(hist, lat, hid, baseline=torch.zeros(d))
    refuses(hist, lat, hid, noise=noise)                                          # together with deterministic=True
    refuses(hist, lat, hid, noise=noise[:, :, :1], deterministic=False)
    refuses(hist, lat, hid, tau=0.0)
    refuses(hist, lat, hid, want=("shift", "soft"))
    refuses(hist, lat, hid, want=())                                              # nothing asked for
    refuses(hist, lat, hid, forecast=True, pos=())
    refuses(hist, lat, hid, forecast=True, pos=(1, d))
    refuses(hist, lat, hid, presence_col=d)
    refuses(hist, lat, hid, max_workspace_mb=1e-4)
    ok = pol.attention_knockout(hist, lat, hid)
    assert ok["latent_shift"].shape == (E, S, nA, N, N)
    # "behavior" is refused by a policy whose GAT reads no behaviour latent; ("history",) works there
    args2 = _e2e_args(device, GAT_use_behavior=False)
    pol2 = Prediction_policy(args2, _Log())
    for sources in (("history", "behavior"), ("behavior",)):
        try:
            pol2.attention_knockout(hist, None, hid, sources=sources)
        except ValueError:
            continue
        raise AssertionError(f"sources={sources} accepted without GAT_use_behavior")
    r = pol2.attention_knockout(hist, None, hid, sources=("history",), want=("latent_ko",))
    h2 = hist.clone()
    h2[..., 2, :] = 0.0
    ref, _ = ops.gat_forward(pol2.gat_arena, h2.to(device).permute(2, 0, 1, 3, 4).reshape(nA, E * S, N, d), None,
                             hid.to(device).permute(2, 0, 1, 3, 4).reshape(nA, E * S, N, A).contiguous(), torch.zeros(nA, E * S, N, N - 1, 2, device=device))
    _sync(device)
    assert same_bits(r["latent_ko"][:, :, :, 2].permute(2, 0, 1, 3, 4).reshape(nA, E * S, N, A), ref)
    return {}
