"""TEST INFRASTRUCTURE: neighbour knock-out through time (csrc/gat_knockout_trace.hip, ops.gat_knockout_trace,
Prediction_policy.attention_knockout_trace) on whatever library is active -- the host emulator in
tests/test_emu_attention_knockout_trace.py, the gfx950 build in tests/test_gpu_attention_knockout_trace.py.

The reference of the bit-for-bit checks is the existing path on an EXPLICIT copy of the episode fields with the knocked entity's rows
replaced in the knocked steps only: ops.gat_trace / attention_trace for the latents and the attention maps, ops.gat_knockout /
attention_knockout for a window of one step, and the plain fp32 torch loop for the distance.  Ground truth of the values:
oracle.gat_forward stepped in fp64 on the same modified fields; error = max|got - ref64| / max|ref64| per (net, job, step) tensor,
bound max(1e-5, E32_FACTOR x the fp32 oracle's own error on the same tensor) at tau = 1, 0.25 and 0.01 -- the rule
attention_checks.assert_vs_fp64 uses for the closed loop (N = 2 at tau = 0.01 is not compared: one gate carries everything there,
DESIGN.md section 5).  The seeds of the fp64 cases were picked with the oracle alone so that the fp32 oracle itself has no gate flip in
the window (no bound >= 0.1); the check asserts it.  The checks never touch ``L.use_library_for_tests``.  Each returns the worst errors."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import knockout_checks as KC
from tests.attention_checks import _bound, _codes, _e2e_args, _gumbel, _sync, _worse
from tests.knockout_checks import KERNEL_CASES, OUTPUTS, bits, host_shift_sq, job_list, same_bits
from tests.oracle_checks import _grad_err, _Log

A = 32
S_STEPS = 5
# (start, D, H) out of S_STEPS: no hand-off; echo; start > 0 with two knocked and two echo steps, ending at S; D = H, no echo; a short
# window ending at S
WINDOWS = [(0, 1, 1), (0, 1, 3), (1, 2, 4), (0, 3, 3), (3, 1, 2)]
# ... at N = 33 and 64 every window has H <= 3 (every step of every job costs a scene and its references)
WINDOWS_LARGE = [(0, 1, 1), (0, 1, 3), (2, 2, 3), (0, 3, 3)]
SAME_BITS_CASES = [c + (w,) for c in KERNEL_CASES for w in (WINDOWS if c[2] <= 17 else WINDOWS_LARGE)]
FP64_WINDOW = {False: (1, 2, 4), True: (3, 1, 2)}                                 # by N > 17 (the fp64 oracle of a step of 64 entities takes a while)
FP64_CASES = [c + (tau,) for c in KERNEL_CASES for tau in (1.0, 0.25, 0.01) if not (c[2] == 2 and tau == 0.01)]
# the seed of every fp64 case: checked on the CPU with the oracle alone (oracle_errors: fp32 against fp64) -- in none of the 17 cases
# has the fp32 oracle a gate flip inside the window (every bound < 0.1; the worst e32 is in profiles/r25_attention_knockout_trace_notes.md)
FP64_SEED = 3


class Case:
    """random GAT parameters; src0 / src1 [n, B, S, N, .] and hidden0 / base are strided views of env-major buffers ([B, S, n, N * w +
    pad] for the step fields) whose surroundings -- the pad floats in front of and behind every scene-step -- are NaN
    (knockout_checks.Case's buffers, extended by a step axis): whatever reads outside its rows poisons its result"""
    knock = KC.Case.knock
    baseline = KC.Case.baseline
    _padded = KC.Case._padded

    def __init__(self, n, B, N, d0, d1, device, S=S_STEPS, seed=0, presence_p=0.8):
        from iplan_amd.arena import ParamArena
        from iplan_amd.config import default_args
        from iplan_amd.nova.GAT_Net import GAT_Net
        self.dims = (n, B, N, d0, d1)
        self.S = S
        self.device = device
        torch.manual_seed(13 + 1000 * n + 100 * B + N + 10 * d0 + d1 + seed)
        args = default_args("highway", use_cuda=False)
        self.mods = [GAT_Net(d0 + d1, args) for _ in range(n)]
        self.params = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.mods]
        self.arena = ParamArena(self.mods, device)
        gen = torch.Generator().manual_seed(seed + 7 * n + 3 * B + N + 5 * S)
        self.src0 = torch.rand(n, B, S, N, d0, generator=gen) * 2 - 1
        self.src0[..., 0] = (torch.rand(n, B, S, N, generator=gen) < presence_p).float()
        self.src1 = torch.softmax(torch.randn(n, B, S, N, d1, generator=gen), -1) * 4 if d1 else None
        self.hidden = torch.randn(n, B, N, A, generator=gen) * 0.1
        self.noise = _gumbel(gen, n, B, S, N, N - 1, 2)
        self.base0 = torch.rand(d0, generator=gen) - 0.5
        self.base1 = torch.softmax(torch.randn(d1, generator=gen), -1) if d1 else None
        self.upload()

    def _padded_steps(self, t, front, back):
        """t [n, B, S, N, w] -> (buffer [B, S, n, front + N w + back] with NaN pads, the view [n, B, S, N, w] into it) on the device"""
        n, B, S, N, w = t.shape
        buf = torch.full((B, S, n, front + N * w + back), float("nan"))
        buf[..., front:front + N * w] = t.permute(1, 2, 0, 3, 4).reshape(B, S, n, N * w)
        buf = buf.to(self.device)
        return buf, buf[..., front:front + N * w].unflatten(-1, (N, w)).permute(2, 0, 1, 3, 4)

    def upload(self):
        dev = self.device
        self.buf0, self.d_src0 = self._padded_steps(self.src0, 3, 2)
        self.buf1, self.d_src1 = self._padded_steps(self.src1, 1, 4) if self.src1 is not None else (None, None)
        self.bufh, self.d_hidden = self._padded(self.hidden, 4, 4)               # (16-byte aligned rows, strides % 4 == 0)
        assert self.d_src0.untyped_storage().nbytes() > 4 * self.d_src0.numel()    # views into larger buffers, not packed copies
        self.d_noise = self.noise.to(dev)
        self.d_base0 = self.base0.to(dev)
        self.d_base1 = self.base1.to(dev) if self.base1 is not None else None

    def window_noise(self, window, noise=True):
        start, _, H = window
        return self.d_noise[:, :, start:start + H].contiguous() if noise else None

    def walk(self, s0, s1, window, noise=True, tau=0.01, hidden=True, want=("latent",), out=None):
        """ops.gat_trace over the window of the fields (s0, s1) [n, B, S, N, .] from the case's hidden state"""
        start, _, H = window
        res = ops.gat_trace(self.arena, s0[:, :, start:start + H], None if s1 is None else s1[:, :, start:start + H],
                            self.d_hidden if hidden else None, self.window_noise(window, noise), tau=tau, want=want, out=out)
        _sync(self.device)
        return res

    def base_walk(self, window, noise=True, tau=0.01, hidden=True):
        """the window with nothing knocked through the existing walk, into a NaN-padded strided buffer -> view [n, B, H, N, A]"""
        n, B, N = self.dims[:3]
        self.buf_base, view = self._padded_steps(torch.zeros(n, B, window[2], N, A), 8, 4)
        self.walk(self.d_src0, self.d_src1, window, noise, tau, hidden, out={"latent": view})
        return view

    def run(self, jobs, window, want=OUTPUTS, noise=True, tau=0.01, knock=None, baseline=False, hidden=True, base=None, out=None):
        start, D, H = window
        if base is None and "shift_sq" in want:
            base = self.base_walk(window, noise, tau, hidden)
        res = ops.gat_knockout_trace(self.arena, self.d_src0, self.d_src1, self.d_hidden if hidden else None, jobs, start=start, duration=D,
                                     horizon=H, base=base, noise=self.window_noise(window, noise), tau=tau, knock=self.knock(knock),
                                     baseline=self.baseline(baseline), want=want, out=out)
        _sync(self.device)
        res["base"] = base
        return res

    def modified(self, j, window, knock=None, baseline=False, device=None):
        """explicit copies (src0, src1) of the fields with entity j's rows replaced in the knocked sources, in the knocked steps only;
        j = -1: plain copies"""
        start, D, _ = window
        k0, k1 = self.knock(knock)
        s0 = self.src0.clone()
        s1 = self.src1.clone() if self.src1 is not None else None
        if j >= 0:
            if k0:
                s0[:, :, start:start + D, j] = self.base0 if baseline else 0.0
            if k1:
                s1[:, :, start:start + D, j] = self.base1 if baseline else 0.0
        if device is not None:
            s0 = s0.to(device)
            s1 = s1.to(device) if s1 is not None else None
        return s0, s1

    def oracle(self, j, window, dtype, noise=True, tau=0.01, knock=None, baseline=False):
        """latents [n, B, H, N, A] of the modified fields in ``dtype``: oracle.gat_forward stepped over the window"""
        n, B, N = self.dims[:3]
        start, _, H = window
        s0, s1 = self.modified(j, window, knock, baseline)
        out = []
        for i in range(n):
            p = {k: v.to(dtype) for k, v in self.params[i].items()}
            h = self.hidden[i].to(dtype).reshape(B * N, A)
            steps = []
            for s in range(start, start + H):
                obs = s0[i, :, s] if s1 is None else torch.cat([s0[i, :, s], s1[i, :, s]], -1)
                nz = (self.noise[i, :, s] if noise else torch.zeros(B, N, N - 1, 2)).to(dtype).reshape(-1, 2)
                h = O.gat_forward(p, obs.to(dtype), h, nz, tau=tau)
                steps.append(h.reshape(B, N, A))
            out.append(torch.stack(steps, 1))
        return torch.stack(out)


# ------------------------------------------------------------------------------------------------ 1: the existing path's bits
def check_same_bits(device, n, B, N, d0, d1, window, noise=True, knock=None, baseline=False, tau=0.01):
    """latent_ko[j] == ops.gat_trace on the modified copy of the fields at every step of the window and attn_ko[j] == its map, job -1
    == the base walk, shift_sq == the fp32 host loop -- all bit for bit; a window of one step == ops.gat_knockout's bits"""
    case = Case(n, B, N, d0, d1, device, seed=1)
    start, D, H = window
    jobs = job_list(N)
    got = case.run(jobs, window, noise=noise, knock=knock, baseline=baseline, tau=tau)
    base = got["base"]
    plain = case.walk(case.d_src0, case.d_src1, window, noise, tau)["latent"]
    assert same_bits(base, plain)
    moved, echo = 0, 0
    for slot, j in enumerate(jobs):
        s0, s1 = case.modified(j, window, knock, baseline, device)
        ref = case.walk(s0, s1, window, noise, tau, want=("latent", "attn"))
        assert same_bits(got["latent_ko"][:, :, slot], ref["latent"]), ("latent_ko differs from gat_trace on the modified copy", j)
        assert same_bits(got["attn_ko"][:, :, slot], ref["attn"]), ("attn_ko differs from the trace's map on the modified copy", j)
        if j < 0:
            assert same_bits(got["latent_ko"][:, :, slot], base), "job -1 differs from the base walk"
        else:
            moved += int(not same_bits(ref["latent"][:, :, :D], base[:, :, :D]))
            echo += int(H > D and not same_bits(ref["latent"][:, :, D:], base[:, :, D:]))
    # (N = 2: one gate per ego carries everything, and at tau = 0.01 a window can find both closed -- nothing to move there)
    assert moved > 0 or N == 2, "no knocked latent differs from the base: the comparison says nothing"
    assert H == D or echo > 0 or N == 2, "no knocked chain differs from the base after the knock: the echo is not exercised"
    host = host_shift_sq(got["latent_ko"], base.unsqueeze(2).expand_as(got["latent_ko"]))
    assert same_bits(got["shift_sq"].cpu(), host), "shift_sq differs from the fp32 host loop"
    assert torch.isfinite(got["latent_ko"]).all() and torch.isfinite(got["shift_sq"]).all() and torch.isfinite(got["attn_ko"]).all()
    if H == 1:
        # no hand-off: the one-step kernel on the same rows and hidden state
        one = ops.gat_knockout(case.arena, case.d_src0[:, :, start], None if case.d_src1 is None else case.d_src1[:, :, start], case.d_hidden,
                               jobs, base=base[:, :, 0], noise=case.d_noise[:, :, start].contiguous() if noise else None, tau=tau,
                               knock=case.knock(knock), baseline=case.baseline(baseline), want=OUTPUTS)
        _sync(device)
        for k in OUTPUTS:
            assert same_bits(got[k][:, :, :, 0], one[k]), (k, "differs from ops.gat_knockout's at a window of one step")
    return {"shift_sq_max": float(got["shift_sq"].max()), "echo_shift_sq_max": float(got["shift_sq"][:, :, :, D:].max()) if H > D else 0.0}


# ------------------------------------------------------------------------------------------------ 2: exact zeros
def check_exact_zeros(device, n, B, N, d0, d1, baseline, window=(1, 2, 4)):
    """entities whose rows already equal the baseline in every knocked step: latent_ko == the base walk bit for bit and shift_sq
    exactly +0.0 at every step of the window, echo steps included"""
    case = Case(n, B, N, d0, d1, device, seed=2)
    start, D, H = window
    quiet = sorted({0, N // 2, N - 1})
    for j in quiet:
        case.src0[:, :, start:start + D, j] = case.base0 if baseline else 0.0
        if d1:
            case.src1[:, :, start:start + D, j] = case.base1 if baseline else 0.0
    case.upload()
    loud = [j for j in range(N) if j not in quiet][:1]
    for noise in (True, False):
        got = case.run(quiet + loud, window, noise=noise, baseline=baseline)
        for slot in range(len(quiet)):
            assert same_bits(got["latent_ko"][:, :, slot], got["base"]), ("rows equal to their baseline moved the latent", quiet[slot])
            assert torch.equal(bits(got["shift_sq"][:, :, slot]), torch.zeros_like(bits(got["shift_sq"][:, :, slot]))), "shift_sq is not +0.0"
        if loud:
            assert (got["shift_sq"][:, :, len(quiet)] > 0).any(), "an informative row moved nothing"
    return {}


# ------------------------------------------------------------------------------------------------ 3: independence and prefix
def check_independence(device, n=2, B=2, N=7, d0=5, d1=3, window=(1, 2, 4)):
    """a slot's bits do not change with the order or length of the job list, duplicates, the other scenes, or the outputs asked for;
    a shorter horizon with the same duration gives a prefix"""
    case = Case(n, B, N, d0, d1, device, seed=4)
    start, D, H = window
    jobs = [3, -1, N - 1, 0]
    ref = case.run(jobs, window)
    base = ref["base"]
    by_job = {j: {k: ref[k][:, :, s] for k in OUTPUTS} for s, j in enumerate(jobs)}

    def agree(got, lst, what, scenes=slice(None), steps=slice(None)):
        for s, j in enumerate(lst):
            for k in OUTPUTS:
                if k in got:
                    assert same_bits(got[k][:, :, s], by_job[j][k][:, scenes, steps]), (what, k, j)
    agree(case.run(jobs[::-1], window, base=base), jobs[::-1], "reversed list")
    agree(case.run([N - 1], window, base=base), [N - 1], "one job")
    agree(case.run([0, 0, 3, 0, -1, -1], window, base=base), [0, 0, 3, 0, -1, -1], "duplicates")
    for want in (("latent_ko",), ("attn_ko",), ("shift_sq",), ("shift_sq", "attn_ko")):
        agree(case.run(jobs, window, want=want, base=base), jobs, want)
    # the other scenes of the launch: one scene alone
    got = ops.gat_knockout_trace(case.arena, case.d_src0[:, 1:], case.d_src1[:, 1:], case.d_hidden[:, 1:], jobs, start=start, duration=D, horizon=H,
                                 base=base[:, 1:], noise=case.window_noise(window)[:, 1:].contiguous(), want=OUTPUTS)
    _sync(device)
    agree(got, jobs, "one scene alone", scenes=slice(1, 2))
    # a shorter horizon: a prefix (of the knocked chains and, through base_walk, of the base walk)
    for h in range(D, H):
        short = case.run(jobs, (start, D, h))
        assert same_bits(short["base"], base[:, :, :h]), ("the base walk of a shorter horizon is no prefix", h)
        agree(short, jobs, ("horizon", h), steps=slice(0, h))
    return {}


# ------------------------------------------------------------------------------------------------ 4: repeatability and ownership
def check_repeatable(device, reps, n=1, B=2, N=17, d0=5, d1=3, window=(1, 2, 4)):
    case = Case(n, B, N, d0, d1, device, seed=5)
    jobs = job_list(N)
    first = case.run(jobs, window)
    for _ in range(reps - 1):
        again = case.run(jobs, window, base=first["base"])
        for k in OUTPUTS:
            assert same_bits(again[k], first[k]), k
    return {}


def check_ownership(device, n, B, N, d0=5, d1=3, window=(1, 2, 3)):
    """outputs as strided views inside sentinel-filled buffers (padded rows, padded step and job slots), inputs inside NaN pads (Case):
    only the owned floats change, every owned float is written, an output not asked for is not written"""
    case = Case(n, B, N, d0, d1, device, seed=6)
    H = window[2]
    jobs = job_list(N)[:4]
    J = len(jobs)
    ref = case.run(jobs, window)
    base_buf = case.buf_base                                                       # (the buffer ref["base"] is a view of)
    base_before = base_buf.cpu().clone()
    shapes = {"latent_ko": (N, A), "attn_ko": (N, N), "shift_sq": (1, N)}

    def carve(k, shift=0.0):
        """a (slot, step)'s [r, c] block is packed (the kernel's layout) and padded behind (a multiple of 4 floats: the latent's
        strides); one step more than H follows every job slot, one job slot more than J every scene, 32 guard floats at either end"""
        r, c = shapes[k]
        cell = r * c + (-(r * c)) % 4 + 8
        body_len = n * B * (J + 1) * (H + 1) * cell
        sent = 0.5 + shift + (torch.arange(body_len + 64, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        view = buf[32:32 + body_len].view(n, B, J + 1, H + 1, cell)[:, :, :J, :H, :r * c].unflatten(-1, (r, c))
        if k == "shift_sq":
            view = view[:, :, :, :, 0]
        own = torch.zeros(body_len + 64, dtype=torch.bool)
        own[32:32 + body_len].view(n, B, J + 1, H + 1, cell)[:, :, :J, :H, :r * c] = True
        return sent, buf, view, own

    for wanted in (OUTPUTS, ("shift_sq",), ("latent_ko", "attn_ko")):
        bufs = {k: carve(k) for k in shapes}
        case.run(jobs, window, want=wanted, base=ref["base"], out={k: bufs[k][2] for k in wanted})
        for k, (sent, buf, view, own) in bufs.items():
            host = buf.cpu()
            if k not in wanted:
                assert torch.equal(bits(host), bits(sent)), (k, "was not asked for and was written")
                continue
            assert same_bits(view, ref[k]), (k, "differs inside a padded buffer")
            assert torch.equal(bits(host[~own]), bits(sent[~own])), (k, "a float outside the owned elements was written")
    b2 = {k: carve(k, 0.25) for k in shapes}
    case.run(jobs, window, base=ref["base"], out={k: b2[k][2] for k in shapes})
    for k in shapes:
        assert same_bits(b2[k][2], ref[k]), (k, "an owned float was left unwritten")
    # every input the kernel reads, and its NaN surroundings, is as it was (the base walk: as the launch in front left it)
    n_, B_, N_ = case.dims[:3]
    for buf, t, front in ((case.buf0, case.src0, 3), (case.buf1, case.src1, 1), (base_buf, ref["base"].cpu(), 8)):
        w = t.shape[3] * t.shape[4]
        host = buf.cpu()
        assert torch.isnan(host[..., :front]).all() and torch.isnan(host[..., front + w:]).all()
        assert same_bits(host[..., front:front + w], t.permute(1, 2, 0, 3, 4).reshape(B_, t.shape[2], n_, w))
    host = case.bufh.cpu()
    assert torch.isnan(host[:, :, :4]).all() and torch.isnan(host[:, :, 4 + N_ * A:]).all()
    assert same_bits(host[:, :, 4:4 + N_ * A], case.hidden.permute(1, 0, 2, 3).reshape(B_, n_, N_ * A))
    assert same_bits(base_buf.cpu(), base_before), "the base walk's buffer was written"
    assert same_bits(case.d_noise.cpu(), case.noise) and same_bits(case.d_base0.cpu(), case.base0)
    return {}


# ------------------------------------------------------------------------------------------------ 5: against fp64
def fp64_case(n, B, N, d0, d1, tau, device="cpu"):
    """the case, window and jobs of an fp64 comparison"""
    case = Case(n, B, N, d0, d1, device, seed=FP64_SEED)
    return case, FP64_WINDOW[N > 17], [j for j in job_list(N) if j >= 0][:3] if N <= 17 else [0, N - 1]


def oracle_errors(case, window, jobs, tau):
    """for noise on / off and every job: (noise, j, fp64 latents [n, B, H, N, A], the fp32 oracle's error per (net, step) [n, H])"""
    n, H = case.dims[0], window[2]
    for noise in (True, False):
        for j in jobs:
            r64, r32 = case.oracle(j, window, torch.float64, noise, tau), case.oracle(j, window, torch.float32, noise, tau)
            e32 = [[_grad_err(r32[i, :, h], r64[i, :, h]) for h in range(H)] for i in range(n)]
            yield noise, j, r64, e32


def check_vs_fp64(device, n, B, N, d0, d1, tau):
    assert not (N == 2 and tau == 0.01)
    case, window, jobs = fp64_case(n, B, N, d0, d1, tau, device)
    H = window[2]
    worst = {"loose_bounds": 0}
    got = {noise: case.run(jobs, window, want=("latent_ko",), noise=noise, tau=tau)["latent_ko"].cpu() for noise in (True, False)}
    b64 = {noise: case.oracle(-1, window, torch.float64, noise, tau) for noise in (True, False)}
    for noise, j, r64, e32 in oracle_errors(case, window, jobs, tau):
        slot = jobs.index(j)
        assert (r64 - b64[noise]).abs().max() > 0, ("the oracle's knocked chain equals its base walk", j)
        for i in range(n):
            for h in range(H):
                err = _grad_err(got[noise][i, :, slot, h], r64[i, :, h])
                print("attention_knockout_trace", (n, B, N, d0, d1), window, "tau", tau, "noise", noise, "job", j, "net", i, "step", h, "err", err,
                      "e32", e32[i][h])
                _worse(worst, f"latent_ko_tau{tau}", err)
                _worse(worst, f"e32_tau{tau}", e32[i][h])
                if _bound(e32[i][h]) >= 0.1:                                       # (an fp32 gate flip: the bound says little there)
                    worst["loose_bounds"] += 1
                assert err <= _bound(e32[i][h]), (tau, noise, j, i, h, err, e32[i][h])
    assert worst["loose_bounds"] == 0, "the fp32 oracle itself has a gate flip in this window: pick another seed (FP64_SEED)"
    return worst


# ------------------------------------------------------------------------------------------------ 6: refusals (entry point and op)
def check_bad_arguments(device):
    """each of these is refused with its code and a message, without a launch; the op refuses on the host"""
    case = Case(1, 2, 5, 5, 3, device, seed=7)
    jobs = [-1, 0, 4]
    window = (1, 2, 3)
    good = case.run(jobs, window)
    nz = case.window_noise(window)
    lib = ops._lib(None)
    a, _, keep = ops.gat_knockout_trace_args(case.arena, case.d_src0, case.d_src1, case.d_hidden, jobs, start=1, duration=2, horizon=3,
                                             base=good["base"], noise=nz, want=OUTPUTS, out={k: good[k] for k in OUTPUTS})
    EINVAL, EALIGN = _codes()

    def refused(code, **fields):
        saved = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        rc = lib.c.iplan_gat_knockout_trace(L.C.byref(a), L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for k, v in saved.items():
            setattr(a, k, v)
        assert rc == code and "iplan_gat_knockout_trace" in msg, (fields, rc, msg)

    def host_jobs(*v):
        arr = (L.C.c_int32 * len(v))(*v)
        keep.append(arr)
        return L.C.cast(arr, L.C.c_void_p)

    rc = lib.c.iplan_gat_knockout_trace(None, L.C.c_void_p(0))
    assert rc == EINVAL and "iplan_gat_knockout_trace" in lib.c.iplan_last_error().decode()
    refused(EINVAL, N=1)
    refused(EINVAL, N=65)
    refused(EINVAL, J=0)
    refused(EINVAL, J=-3)
    refused(EINVAL, H=0)
    refused(EINVAL, H=-1)
    refused(EINVAL, D=0)
    refused(EINVAL, D=4)                                                           # D > H
    refused(EINVAL, start=-1)
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
    refused(EALIGN, lat_s_step=a.lat_s_step + 2)
    refused(EALIGN, hidden0=case.d_hidden.data_ptr() + 4)
    refused(EALIGN, h_s_b=a.h_s_b + 2)
    lib.call("iplan_gat_knockout_trace", a, L.current_stream(device))              # the descriptor itself is good
    _sync(device)
    again = case.run(jobs, window, base=good["base"])
    for k in OUTPUTS:
        assert same_bits(again[k], good[k]), k

    def op_refuses(**kw):
        args = dict(jobs=jobs, start=1, duration=2, horizon=3, base=good["base"], noise=nz, want=OUTPUTS)
        args.update(kw)
        j = args.pop("jobs")
        try:
            ops.gat_knockout_trace(case.arena, case.d_src0, args.pop("src1", case.d_src1), case.d_hidden, j, **args)
        except AssertionError:
            return
        raise AssertionError(f"ops.gat_knockout_trace accepted {kw}")
    op_refuses(jobs=[])
    op_refuses(jobs=[5])
    op_refuses(jobs=[-2])
    op_refuses(want=())
    op_refuses(want=("latent",))
    op_refuses(base=None)
    op_refuses(base=good["base"][:, :, :2])                                       # the base walk of another window
    op_refuses(src1=None, knock=(True, True))
    op_refuses(baseline=(case.d_base0[:3], None))
    op_refuses(start=-1)
    op_refuses(start=3)                                                            # start + H > S
    op_refuses(horizon=0)
    op_refuses(duration=0)
    op_refuses(duration=4)
    op_refuses(noise=case.d_noise)                                                 # the whole episode's, not the window's
    op_refuses(out={"latent_ko": torch.empty(1, 2, 3, 3, 5, A, device=device)[..., :16]})
    op_refuses(out={"shift_sq": torch.empty(1, 2, 4, 3, 5, device=device)})    # a job slot too many
    op_refuses(out={"shift_sq": torch.empty(1, 2, 3, 4, 5, device=device)})    # a step too many
    return {}


# ------------------------------------------------------------------------------------------------ 7: the method
WANT_ALL = ("shift", "latent_ko", "attention_ko")


def _method_inputs(args, E, S, seed):
    from iplan_amd import synth
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    gen = torch.Generator().manual_seed(seed)
    hist = synth.make_history(gen, (E, S, nA), N, d, presence_p=0.7)
    lat = torch.softmax(torch.randn(E, S, nA, N, Z, generator=gen), -1)
    hid0 = torch.randn(E, nA, N, A, generator=gen) * 0.1
    noise = _gumbel(gen, nA, E, S, N, N - 1, 2)
    return hist, lat, hid0, noise


def host_summary(shift, hist, jobs, start, D, presence_col=0):
    """float64 numpy restatement of ``summary``: shift [E,H,nA,N,J], hist [E,S,nA,N,d] -> [nA, H, 2]"""
    shift = np.asarray(shift, dtype=np.float64)
    hist = np.asarray(hist)
    E, H, nA, N, J = shift.shape
    pres = hist[..., presence_col] != 0 if presence_col >= 0 else np.ones(hist.shape[:4], dtype=bool)      # [E, S, nA, N]
    out = np.full((nA, H, 2), np.nan)
    for a in range(nA):
        for h in range(H):
            tot, cnt = [0.0, 0.0], [0, 0]
            for e in range(E):
                for i in range(N):
                    for s, j in enumerate(jobs):
                        if pres[e, start + h, a, i] and pres[e, start:start + D, a, j].any():
                            tot[int(i == j)] += shift[e, h, a, i, s]
                            cnt[int(i == j)] += 1
            for col in range(2):
                if cnt[col]:
                    out[a, h, col] = tot[col] / cnt[col]
    return out


def check_methods(device, tmp_path, E, S, N=5):
    """attention_knockout_trace on a loaded checkpoint: numpy and device round trips, every result against the existing methods on
    explicit copies, chunked == unchunked, a window of one step == attention_knockout, the sources and baselines, summary"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device, max_vehicle_num=N)
    pol, _, _ = _loaded_policy(args, tmp_path, 23)
    nA, d, Z = args.n_agents, args.obs_shape_single, args.latent_dim
    hist, lat, hid0, noise = _method_inputs(args, E, S, 8)
    hist[:, :, :, 1] = 0.0                                                         # a vehicle never seen: knocking it changes nothing
    lat[:, :, :, 1] = 0.0
    dv = lambda t: t.to(device)                                                    # noqa: E731
    start, D = (1, 1) if S >= 3 else (0, 1)
    H = S - start
    nzw = noise[:, :, start:start + H].contiguous()
    kw = dict(start=start, duration=D, deterministic=False, want=WANT_ALL)
    r_np = pol.attention_knockout_trace(hist.double().numpy(), lat.numpy(), hid0.numpy(), noise=nzw.numpy(), **kw)
    r_dev = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), **kw)
    per_env = 4 * nA * H * (2 * N * (N - 1) + N * A)
    per_job = 4 * nA * H * (N + N * A + N * N)
    tiny = (per_env + 2 * per_job + 8) / (1 << 20)                                 # one environment and two of the five jobs per chunk
    r_chunk = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), max_workspace_mb=tiny, **kw)
    _sync(device)
    shapes = {"latent": (E, H, nA, N, A), "latent_shift": (E, H, nA, N, N), "latent_ko": (E, H, nA, N, N, A), "attention_ko": (E, H, nA, N, N, N)}
    for k, shape in shapes.items():
        assert isinstance(r_np[k], np.ndarray) and r_np[k].shape == shape and r_np[k].dtype == np.float32, (k, r_np[k].shape)
        assert torch.is_tensor(r_dev[k]) and r_dev[k].device.type == torch.device(device).type and r_dev[k].shape == shape, k
        assert np.array_equal(r_dev[k].cpu().numpy().view(np.int32), r_np[k].view(np.int32)), (k, "numpy and device round trips differ")
        assert same_bits(r_chunk[k], r_dev[k]), (k, "chunked and unchunked calls differ")
    for r in (r_np, r_dev, r_chunk):
        assert np.array_equal(r["knocked"], np.arange(N)) and r["summary"].shape == (nA, H, 2) and r["summary"].dtype == np.float64
        assert r["window"] == (start, D, H) and r["sources"] == ("history", "behavior")
        assert np.array_equal(r["summary"], r_np["summary"], equal_nan=True)
    # against attention_trace on explicit copies of the fields
    tr = pol.attention_trace(dv(hist[:, start:]), dv(lat[:, start:]), hidden0=dv(hid0), noise=dv(nzw), want=("attention",), _stats=False)
    assert same_bits(r_dev["latent"], tr["latent"]), "latent != attention_trace's on the window"
    for j in range(N):
        h2, l2 = hist.clone(), lat.clone()
        h2[:, start:start + D, :, j] = 0.0
        l2[:, start:start + D, :, j] = 0.0
        tr = pol.attention_trace(dv(h2[:, start:]), dv(l2[:, start:]), hidden0=dv(hid0), noise=dv(nzw), want=("attention",), _stats=False)
        _sync(device)
        assert same_bits(r_dev["latent_ko"][:, :, :, j], tr["latent"]), ("latent_ko != attention_trace on the modified copy", j)
        assert same_bits(r_dev["attention_ko"][:, :, :, j], tr["attention"]), ("attention_ko != attention_trace's map on the modified copy", j)
    # latent_shift: torch's sqrt (on the device the method ran on) of the fp32 host loop
    ko, base = r_dev["latent_ko"].cpu(), r_dev["latent"].cpu()
    sq = host_shift_sq(ko, base.unsqueeze(3).expand_as(ko))                        # [E, H, nA, J, N]
    assert same_bits(r_dev["latent_shift"].cpu(), sq.to(device).sqrt().cpu().transpose(3, 4)), "latent_shift != torch's sqrt of the host loop"
    same = (bits(ko) == bits(base.unsqueeze(3).expand_as(ko))).all(-1).transpose(3, 4)      # [E, H, nA, N(ego), J]
    assert same[..., 1].all(), "knocking the vehicle never seen moved a latent"
    assert (r_dev["latent_shift"].cpu()[same] == 0).all() and (r_dev["latent_shift"] > 0).any()
    if H > D:
        assert (r_dev["latent_shift"][:, D:] > 0).any(), "no echo after the knock: the carried latent is not exercised"
    # summary against its float64 restatement
    ref = host_summary(r_np["latent_shift"], hist.numpy(), list(range(N)), start, D)
    assert np.allclose(r_np["summary"], ref, rtol=1e-12, atol=0, equal_nan=True), (r_np["summary"], ref)
    assert np.isnan(ref).sum() < ref.size
    every = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), start=start, duration=D, presence_col=-1)
    ref = host_summary(every["latent_shift"].cpu().numpy(), hist.numpy(), list(range(N)), start, D, presence_col=-1)
    assert np.allclose(every["summary"], ref, rtol=1e-12, atol=0) and not np.isnan(ref).any()
    # a window of one step: attention_knockout's on the same row and hidden state, bit for bit
    for s0 in (0, S - 1):
        one = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), start=s0, duration=1, horizon=1, noise=dv(noise[:, :, s0:s0 + 1].contiguous()),
                                           deterministic=False, want=WANT_ALL)
        ak = pol.attention_knockout(dv(hist[:, s0:s0 + 1]), dv(lat[:, s0:s0 + 1]), dv(hid0).unsqueeze(1), noise=dv(noise[:, :, s0:s0 + 1].contiguous()),
                                    deterministic=False, want=WANT_ALL)
        for k in shapes:
            assert same_bits(one[k], ak[k]), (k, "a window of one step differs from attention_knockout", s0)
    det = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), start=0, duration=1, horizon=1)
    ak = pol.attention_knockout(dv(hist[:, :1]), dv(lat[:, :1]), dv(hid0).unsqueeze(1))
    assert same_bits(det["latent_shift"], ak["latent_shift"]) and same_bits(det["latent"], ak["latent"]), "deterministic: differs from attention_knockout"
    # the sources, a baseline, a subset of entities with a duplicate, hidden0 = None, tau, duration = None
    base_rows = (torch.rand(d) - 0.5, torch.softmax(torch.randn(Z), -1))
    ents = [3, 0, 3]
    for sources, baseline in ((("behavior",), None), (("history",), None), (("history", "behavior"), base_rows), ("behavior", (None, base_rows[1]))):
        r = pol.attention_knockout_trace(dv(hist), dv(lat), None, entities=ents, sources=sources, baseline=baseline, duration=None,
                                         want=("shift", "latent_ko"), tau=0.25)
        src = (sources,) if isinstance(sources, str) else sources
        assert r["latent_shift"].shape == (E, S, nA, N, 3) and np.array_equal(r["knocked"], ents) and r["window"] == (0, S, S) and r["sources"] == src
        for slot, j in enumerate(ents[:2]):
            h2, l2 = hist.clone(), lat.clone()
            if "history" in src:
                h2[..., j, :] = 0.0 if baseline is None or baseline[0] is None else baseline[0]
            if "behavior" in src:
                l2[..., j, :] = 0.0 if baseline is None or baseline[1] is None else baseline[1]
            refl = ops.gat_trace(pol.gat_arena, dv(h2).permute(2, 0, 1, 3, 4), dv(l2).permute(2, 0, 1, 3, 4), None, None, tau=0.25)["latent"]
            _sync(device)
            assert same_bits(r["latent_ko"][:, :, :, slot].permute(2, 0, 1, 3, 4), refl), (sources, "latent_ko differs from gat_trace on the modified copy", j)
        assert same_bits(r["latent_ko"][:, :, :, 0], r["latent_ko"][:, :, :, 2]), "a duplicate entity gave other bits"
    # ``want`` is honoured: without "shift" no distance and no summary, and the other results keep their bits
    only = pol.attention_knockout_trace(dv(hist), dv(lat), dv(hid0), noise=dv(nzw), start=start, duration=D, deterministic=False, want=("latent_ko",))
    assert set(only) == {"latent", "latent_ko", "knocked", "sources", "window"}, sorted(only)
    assert same_bits(only["latent_ko"], r_dev["latent_ko"]) and same_bits(only["latent"], r_dev["latent"])
    return {"latent_shift_max": float(r_np["latent_shift"].max()),
            "echo_shift_max": float(r_np["latent_shift"][:, D:].max()) if H > D else 0.0}


def check_nothing_touched(device, tmp_path, reps):
    """the call touches no parameter, gradient entry, optimiser state or input; in the deterministic mode no generator; ``reps`` calls agree"""
    from tests.predict_checks import _loaded_policy
    args = _e2e_args(device)
    pol, _, _ = _loaded_policy(args, tmp_path, 29)
    hist, lat, hid0, _ = _method_inputs(args, 2, 3, 9)
    dv = lambda t: t.to(device)                                                    # noqa: E731
    pol.gat_arena.grad.normal_()
    pol.dec_arena.grad.normal_()
    before = dict(gat=pol.gat_arena.data.clone(), dec=pol.dec_arena.data.clone(), ggat=pol.gat_arena.grad.clone(), gdec=pol.dec_arena.grad.clone(),
                  opt=[str(o.state_dict()) for o in pol.pred_optimizer])
    states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None, np.random.get_state()[1].copy())
    inputs = [dv(hist), dv(lat), dv(hid0)]
    copies = [t.clone() for t in inputs]
    first = pol.attention_knockout_trace(*inputs, want=WANT_ALL)
    for _ in range(reps - 1):
        again = pol.attention_knockout_trace(*inputs, want=WANT_ALL)
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
    own = pol.attention_knockout_trace(*inputs, deterministic=False)
    assert torch.isfinite(own["latent_shift"]).all()
    return {}


def check_learn_unaffected(device, E=2):
    """learn() with injected sel / noise / keep gives the same loss and parameters whether or not an attention_knockout_trace ran before it"""
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
            r = pol.attention_knockout_trace(D["history"][:, 1:5], D["behavior_latent"][:, :4], D["attention_latent"][:, 1], start=1, duration=1)
            assert torch.isfinite(r["latent_shift"]).all() and r["latent_shift"].shape[1] == 3
        losses = pol.learn(batch, 0, noise=noise, keep=keep, sel=sel)
        _sync(device)
        results.append((np.asarray(losses), pol.gat_arena.data.clone(), pol.dec_arena.data.clone()))
    (l0, g0, d0), (l1, g1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(g0, g1) and torch.equal(d0, d1)
    return {}


def check_method_refusals(device):
    """every refusal of attention_knockout_trace raises ValueError before anything is launched"""
    from iplan_amd.nova.prediction_policy import Prediction_policy
    args = _e2e_args(device)
    pol = Prediction_policy(args, _Log())
    E, S = 1, 3
    nA, N, d, Z = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim
    hist, lat, hid0, noise = _method_inputs(args, E, S, 10)

    def refuses(*a, **kw):
        try:
            pol.attention_knockout_trace(*a, **kw)
        except ValueError:
            return
        raise AssertionError(f"attention_knockout_trace accepted {kw}")
    refuses(hist[:, 0], lat, hid0)
    refuses(hist[:, :, :1], lat, hid0)
    refuses(hist[..., :3], lat, hid0)
    refuses(hist, None, hid0)
    refuses(hist, lat[:, :1], hid0)
    refuses(hist, lat, hid0[..., :16])
    refuses(hist, lat, hid0.unsqueeze(1))
    refuses(hist, lat, hid0, entities=[])
    refuses(hist, lat, hid0, entities=[N])
    refuses(hist, lat, hid0, entities=[-1])
    refuses(hist, lat, hid0, entities=[0.5])
    refuses(hist, lat, hid0, entities=3)
    refuses(hist, lat, hid0, sources=())
    refuses(hist, lat, hid0, sources=("history", "intent"))
    refuses(hist, lat, hid0, baseline=(torch.zeros(d + 1), None))
    refuses(hist, lat, hid0, baseline=(None, torch.zeros(Z - 1)))
    refuses(hist, lat, hid0, baseline=torch.zeros(d))
    refuses(hist, lat, hid0, noise=noise)                                         # together with deterministic=True
    refuses(hist, lat, hid0, noise=noise, start=1, deterministic=False)           # the whole episode's, not the window's
    refuses(hist, lat, hid0, tau=0.0)
    refuses(hist, lat, hid0, want=("shift", "soft"))
    refuses(hist, lat, hid0, want=())                                             # nothing asked for
    refuses(hist, lat, hid0, presence_col=d)
    refuses(hist, lat, hid0, start=-1)
    refuses(hist, lat, hid0, start=S)
    refuses(hist, lat, hid0, start=0.0)
    refuses(hist, lat, hid0, horizon=0)
    refuses(hist, lat, hid0, horizon=S + 1)
    refuses(hist, lat, hid0, start=1, horizon=S)                                  # start + H > S
    refuses(hist, lat, hid0, horizon=2.0)
    refuses(hist, lat, hid0, duration=0)
    refuses(hist, lat, hid0, duration=S + 1)
    refuses(hist, lat, hid0, horizon=2, duration=3)
    refuses(hist, lat, hid0, max_workspace_mb=1e-4)
    ok = pol.attention_knockout_trace(hist, lat, hid0)
    assert ok["latent_shift"].shape == (E, S, nA, N, N) and ok["window"] == (0, 1, S)
    # "behavior" is refused by a policy whose GAT reads no behaviour latent; ("history",) works there
    args2 = _e2e_args(device, GAT_use_behavior=False)
    pol2 = Prediction_policy(args2, _Log())
    for sources in (("history", "behavior"), ("behavior",)):
        try:
            pol2.attention_knockout_trace(hist, None, hid0, sources=sources)
        except ValueError:
            continue
        raise AssertionError(f"sources={sources} accepted without GAT_use_behavior")
    r = pol2.attention_knockout_trace(hist, None, hid0, sources=("history",), want=("latent_ko",))
    h2 = hist.clone()
    h2[:, :1, :, 2, :] = 0.0
    ref = pol2.attention_trace(h2.to(device), None, hidden0=hid0.to(device), deterministic=True, _stats=False)["latent"]
    _sync(device)
    assert same_bits(r["latent_ko"][:, :, :, 2], ref)
    return {}
