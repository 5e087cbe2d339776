"""TEST INFRASTRUCTURE: the behaviour learning kernels alone (csrc/behavior_learn.hip through ops.beh_forward + ops.beh_backward and
ops.bdec_forward) on whatever library is active -- the host emulator in tests/test_emu_behavior_learn.py, the gfx950 build in
tests/test_gpu_behavior_learn.py.

Reference: fp64 autograd of oracle.behavior_learn_loss (oracle.behavior_hard_learn_loss for the hard update), per net, on the same
inputs, with the fp32 evaluation beside it.  The loop is restated here window by window (``_net_reference``) because the checks need
what the oracle functions do not return -- the predictions, for the distance of the draw from the loss's kinks, the ReLU
pre-activations, and an injected normaliser -- and ``check_restatement`` holds the restatement to the oracle functions bit for bit.
Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor (``_grad_err``), bound = max(1e-5, E32_FACTOR x e32),
e32 = the fp32 reference's own error against fp64 OF THAT TENSOR; a tensor whose fp64 reference is exactly zero must be exactly zero.
Unclipped gradients of every encoder and decoder parameter of every net, and both loss components, are compared.

The loss has three kinds of kink -- |next - pred|, the ReLU of the two input Linears, clamp(||curr - pred|| - thres, 0) under a
penalty -- and no case may sit on one: every reference asserts min |next - pred| > KINK_MARGIN over the masked-in entries,
min | ||curr - pred|| - thres | > KINK_MARGIN under a penalty, and the same branch at every ReLU in fp32 and fp64.  A draw that fails
gets another seed (BEH_SEEDS, found on the CPU from the references alone); nothing is masked out.
The checks never touch ``L.use_library_for_tests``: the caller decides which library is active.  Each returns the worst errors it saw."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import behavior_eval_checks as BC
from tests.kernel_checks import KINK_MARGIN, _bits_equal, _param_slots, _refused, _rehome_grads
from tests.oracle_checks import E32_FACTOR, _grad_err, _req

TOL = 1e-5
COEF, THRES = BC.COEF, BC.THRES
DROP_P = 0.1
PENALTY, PENALTY_THRES = 0.3, 0.05
NORM_FACTOR = 1.7
FORMS_CLOSE_V1_V2 = 3e-6        # first against second form, worst gradient error (tests/test_emu_learners.py: ..._both_forms_emulated)
FORMS_CLOSE_ROWS = 1e-6         # IPLAN_DEC_THIN_ROWS against IPLAN_DEC_BWD_V1: the same contraction kernels

# (E, N, L, J, d, Z, n_nets), T = J + 1 + L.
# rows E * N one below, at and one past a 16-row tile; 48 = a decoder workgroup's three tiles exactly; 49 = 4 tiles, decoder workgroups
# 3 + 1 with a one-row ragged tile, the encoder's 4-tile workgroup exactly full; 65 = 5 tiles, encoder workgroups 4 + 1; 97 = 7 tiles,
# decoder workgroups 3 + 3 + 1: three thin-gradient partials.  N = 5, 7, 12, 13 put env boundaries inside a tile.
ROW_CASES = [(1, 1, 2, 3, 5, 8, 1), (3, 5, 2, 3, 5, 8, 2), (2, 8, 2, 3, 5, 8, 5), (1, 17, 2, 3, 5, 8, 2), (4, 12, 2, 3, 5, 8, 1),
             (7, 7, 2, 3, 5, 8, 2), (5, 13, 2, 3, 5, 8, 5), (1, 97, 2, 3, 5, 8, 1)]
# 17 rows; (8, 8) is the last width on the decoder forward's second form, (9, 7) the first one off it
WIDTH_CASES = [(1, 17, 2, 3, d, Z, 2 if (d, Z) in ((8, 8), (9, 7)) else 1) for d, Z in ((1, 15), (4, 1), (8, 8), (9, 7), (12, 4), (15, 1))]
# J = 1; L = 1; L = 10 with J = 2 (curr still padded in every window); J = L + 3; J = 26 at L = 1 (short first window range)
WINDOW_CASES = [(3, 5, 2, 1, 5, 8, 2), (3, 5, 1, 3, 5, 8, 2), (1, 17, 10, 2, 5, 8, 1), (3, 5, 2, 5, 5, 8, 2), (1, 17, 1, 26, 5, 8, 1)]
SHORT_RANGE_CASE = WINDOW_CASES[-1]
LONG_CASE = (1, 2, 1, 513, 5, 8, 1)                      # more than BEH_D2_MAX_WINDOWS windows (the gfx950 suite only)
MASK_CASE = (3, 5, 2, 3, 5, 8, 2)
MASK_KINDS = ("random", "ones", "zero_window", "zero_net")
FORM_SHAPES = {17: (1, 17, 2, 3, 5, 8, 2), 49: (7, 7, 2, 3, 5, 8, 2), 97: (1, 97, 2, 3, 5, 8, 1)}
# the accumulating form splits the ENVS in two shards and the 17- and 97-row form shapes hold one env: it runs at 2 x 9 = 18, 7 x 7 =
# 49 and 2 x 49 = 98 rows -- the form shapes' 2, 4 and 7 tiles, entities per env kept above one so that a shard's env boundary falls
# inside a tile (17 x 1 and 97 x 1 would split as well, with every row an env of its own)
ACC_SHAPES = {17: (2, 9, 2, 3, 5, 8, 2), 49: (7, 7, 2, 3, 5, 8, 2), 97: (2, 49, 2, 3, 5, 8, 1)}
# form -> (environment knobs, launch / reference options)
FORMS = {
    "default": ({}, {}),
    "dec_fwd_v1": ({"IPLAN_DEC_FWD_V1": "1"}, {}),
    "dec_bwd_v1": ({"IPLAN_DEC_BWD_V1": "1"}, {}),
    "dec_thin_rows": ({"IPLAN_DEC_THIN_ROWS": "1"}, {}),
    "enc_fp32": ({"IPLAN_ENC_FP32": "1"}, {}),
    "fwd_save_act": ({"IPLAN_FWD_SAVE_ACT": "1"}, {}),
    "pieces_1": ({"IPLAN_BEH_PIECES": "1"}, {}),
    "pieces_3": ({"IPLAN_BEH_PIECES": "3"}, {}),
    "pieces_3_equal": ({"IPLAN_BEH_PIECES": "3", "IPLAN_BEH_EQUAL_PIECES": "1"}, {}),
    "serial": ({"IPLAN_BEH_SERIAL": "1"}, {}),
    "hard": ({}, dict(hard=True)),
    "penalty": ({}, dict(penalty=PENALTY, thres=PENALTY_THRES)),
    "penalty_dec_bwd_v1": ({"IPLAN_DEC_BWD_V1": "1"}, dict(penalty=PENALTY, thres=PENALTY_THRES)),
    "defer_dec_wgrad": ({}, dict(defer=True)),
    "accumulate": ({}, dict(shards=True)),
    "win_norm": ({}, dict(norm_factor=NORM_FACTOR)),
}
# seeds at which a case's draw keeps off every kink under every option it runs with (found on the CPU from the references alone; 0
# where not listed)
BEH_SEEDS = {
    "E1_N17_L2_J3_d12_Z4_n1_random": 1,
    "E1_N2_L1_J513_d5_Z8_n1_random": 1,
    "E1_N97_L2_J3_d5_Z8_n1_random": 1,
    "E5_N13_L2_J3_d5_Z8_n5_random": 1,
    "E7_N7_L2_J3_d5_Z8_n2_random": 2,
}


def case_id(E, N, Lw, J, d, Z, n_nets, mask_kind="random"):
    return f"E{E}_N{N}_L{Lw}_J{J}_d{d}_Z{Z}_n{n_nets}_{mask_kind}"


_sync, _worse = BC._sync, BC._worse


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


# ------------------------------------------------------------------------------------------------ the seeded dropout draw
def keep_hash_np(seed, idx):
    """keep_hash of csrc/behavior_learn.hip on an array of 64-bit element indices, in 32-bit arithmetic"""
    u = np.uint64
    m32 = u(0xFFFFFFFF)
    idx = np.asarray(idx, dtype=np.uint64)

    def mul(x, c):
        return (x * u(c)) & m32
    x = (idx & m32) ^ mul(idx >> u(32), 0x9E3779B9) ^ u(seed & 0xFFFFFFFF)
    x = x ^ (x >> u(16))
    x = mul(x, 0x85EBCA6B)
    x = x ^ (x >> u(13))
    x = mul(x, 0xC2B2AE35)
    x = x ^ (x >> u(16))
    x = x ^ u((seed >> 32) & 0xFFFFFFFF)
    x = x ^ (x >> u(15))
    x = mul(x, 0x2C1B3C6D)
    x = x ^ (x >> u(12))
    return x


def keep_threshold(p):
    return int(np.uint32(np.float32(p) * np.float32(65536.0)))


def seeded_keep(seed, p, shape):
    """the keep flags the kernels draw for ``seed`` over the linear element index of a [n_nets, J, rows, L, 64] tensor: element i uses
    the hash of i & ~1, its low 16 bits where i is even and its high 16 bits where i is odd; kept iff that is >= uint32(float32(p) *
    65536) (keep_flags4 / keep_tile of csrc/behavior_learn.hip)"""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64)
    h = keep_hash_np(seed, i & ~np.uint64(1))
    u16 = np.where((i & np.uint64(1)) == 0, h & np.uint64(0xFFFF), h >> np.uint64(16))
    return (u16 >= np.uint64(keep_threshold(p))).astype(np.uint8).reshape(shape)


# ------------------------------------------------------------------------------------------------ cases and references
class LearnCase(BC.Case):
    """behavior_eval_checks.Case (strided [net, E, T, N, d] view, per-net random parameters and arenas, masks with a zero
    mid-episode) with the mask kinds of this suite -- "random", "ones", "zero_window" (the target steps of window 1, or of window 0
    when there is only one, zero in every env), "zero_net" (net 0 of several all zeros) -- and Bernoulli(1 - DROP_P) keep flags"""

    def __init__(self, E, N, Lw, J, d, Z, n_nets, device, mask_kind="random", seed=None):
        self.id = case_id(E, N, Lw, J, d, Z, n_nets, mask_kind)
        self.seed = BEH_SEEDS.get(self.id, 0) if seed is None else seed
        self.mask_kind = mask_kind
        super().__init__(E, N, Lw, J, d, Z, n_nets, device, seed=self.seed)
        if mask_kind == "ones":
            self.mask[:] = 1.0
        elif mask_kind == "zero_window":
            j0 = min(1, J - 1)
            self.mask[:, :, j0 + 1:j0 + 1 + Lw] = 0.0
        elif mask_kind == "zero_net":
            assert n_nets > 1
            self.mask[0] = 0.0
        else:
            assert mask_kind == "random"
        self.rows = E * N
        self._keeps = {}
        self.upload()

    def windows(self, hard=False):
        return (self.T // self.L - 1) if hard else self.J

    def keep(self, hard=False):
        """uint8 [n_nets, J, rows, L, 64] on the CPU (its own J under the hard update)"""
        if hard not in self._keeps:
            gen = torch.Generator().manual_seed(977 + self.seed + self.rows + (1 if hard else 0))
            self._keeps[hard] = (torch.rand(self.n_nets, self.windows(hard), self.rows, self.L, 64, generator=gen) < 1.0 - DROP_P).to(torch.uint8)
        return self._keeps[hard]

    def win_norm(self, hard=False, factor=1.0):
        """float32 [n_nets, J] on the CPU: ``factor`` x the mask's own per-window sums"""
        return (ops.beh_window_mask_sums(self.mask, self.L, hard) * factor).contiguous()


def _net_reference(case, n, dtype, hard=False, keep=None, drop_p=0.0, penalty=0.0, thres=THRES, win_norm=None):
    """net n: the loop of oracle.behavior_learn_loss / behavior_hard_learn_loss, the same operations in the same order, with the
    predictions and the ReLU pre-activations looked at on the way.  ``keep`` [J, rows, L, 64] or None; ``win_norm`` [J] (soft update
    only): the normaliser of window j is win_norm[j] * N * d instead of the window's own mask sum.
    Returns dict(beh, stab, enc={name: grad}, dec={name: grad}, l1_margin, stab_margin, relu=bool tensor of every ReLU branch)."""
    E, N, Lw, d, Z, T = case.E, case.N, case.L, case.d, case.Z, case.T
    hist = case.view(case.buf)[n].to(dtype)
    mask = case.mask[n]
    ep, dpf = _req(case.enc_p[n], dtype), _req(case.dec_p[n], dtype)
    dp = O.strip_prefix(dpf, "decoder.")
    drop = None if keep is None else keep.to(dtype)
    latent = torch.zeros(E, N, Z, dtype=dtype)
    eh, dh = torch.zeros(E * N, 32, dtype=dtype), torch.zeros(E * N, 64, dtype=dtype)
    relu, l1_margin, stab_margin = [], float("inf"), float("inf")

    def look(curr, dec_in, pred, nxt, mn):
        nonlocal l1_margin, stab_margin
        with torch.no_grad():
            relu.append((dec_in.reshape(E * N, Lw, d + Z) @ dp["linear.weight"].t() + dp["linear.bias"] > 0).flatten())
            relu.append((curr.reshape(E * N, Lw, d) @ ep["linear.weight"].t() + ep["linear.bias"] > 0).flatten())
            gap = (nxt - pred).abs()[mn > 0]
            if gap.numel():
                l1_margin = min(l1_margin, float(gap.min()))
            if penalty != 0.0:
                stab_margin = min(stab_margin, float((torch.linalg.norm(curr - pred, dim=-1) - thres).abs().min()))

    if hard:
        assert win_norm is None and penalty == 0.0
        nh = T // Lw
        J = nh - 1
        blocks = hist[:, :nh * Lw].reshape(E, nh, Lw, N, d)
        m_all = mask[:, :J * Lw].to(dtype)
        preds = []
        for j in range(J):
            curr = blocks[:, j].permute(0, 2, 1, 3)
            dec_in = torch.cat([curr, latent[:, :, None, :].expand(E, N, Lw, Z)], dim=-1)
            pred, dh = O.decoder_forward(dp, dec_in.reshape(E * N, Lw, d + Z), dh, None if drop is None else drop[j], drop_p)
            preds.append(pred.reshape(E, N, Lw, d).permute(0, 2, 1, 3))
            look(curr, dec_in, pred.reshape(E, N, Lw, d), blocks[:, j + 1].permute(0, 2, 1, 3),
                 m_all[:, j * Lw:(j + 1) * Lw, None, None].expand(E, Lw, N, d).permute(0, 2, 1, 3))
            _, eh, latent = O.encoder_forward(ep, curr.reshape(E * N, Lw, d), eh)
            latent = latent.reshape(E, N, Z)
        nxt = blocks[:, 1:].reshape(E, J * Lw, N, d)
        pred = torch.stack(preds, 1).reshape(E, J * Lw, N, d)
        m = m_all[:, :, None, None].expand(E, J * Lw, N, d)
        beh = (torch.abs(nxt - pred) * m).sum() / (m.sum() + O.EPS) * d * N
        stab = torch.zeros((), dtype=dtype)
        loss = beh
    else:
        J = T - 1 - Lw
        beh, stab = 0.0, 0.0
        for j in range(J):
            curr, nxt, mn = O.behavior_windows(hist, mask, j, Lw)
            dec_in = torch.cat([curr, latent[:, :, None, :].expand(E, N, Lw, Z)], dim=-1)
            pred, dh = O.decoder_forward(dp, dec_in.reshape(E * N, Lw, d + Z), dh, None if drop is None else drop[j], drop_p)
            pred = pred.reshape(E, N, Lw, d)
            look(curr, dec_in, pred, nxt, mn)
            _, eh, new_lat = O.encoder_forward(ep, curr.reshape(E * N, Lw, d), eh)
            st = torch.linalg.norm(curr - pred, dim=-1).reshape(-1)
            latent = (1.0 - COEF) * latent + new_lat.reshape(E, N, Z) * COEF
            if win_norm is None:
                beh = beh + O.masked_l1(nxt, pred, mn, d * N)
            else:
                beh = beh + (torch.abs(nxt - pred) * mn).sum() / (win_norm[j].to(dtype) * (N * d) + O.EPS) * (d * N)
            stab = stab + torch.clamp(st - thres, min=0).sum() / E / Lw
        beh = beh / J
        stab = stab / J
        loss = beh + penalty * stab
    loss.backward()
    def grads(p):                                              # (a parameter the loss does not reach -- the encoder at J = 1 -- has gradient 0)
        return {k: torch.zeros_like(v) if v.grad is None else v.grad for k, v in p.items()}
    return dict(beh=beh.detach().reshape(1), stab=stab.detach().reshape(1), enc=grads(ep), dec=grads(dpf),
                l1_margin=l1_margin, stab_margin=stab_margin, relu=torch.cat(relu))


_REFS = {}


def reference(case, hard=False, drop=False, penalty=0.0, thres=THRES, norm_factor=None):
    """(fp64, fp32) lists of per-net references, computed once per (case, options) and shared between the checks; asserts that the draw
    keeps off the kinks"""
    key = (case.id, case.seed, hard, drop, penalty, thres, norm_factor)
    if key not in _REFS:
        keep = case.keep(hard) if drop else None
        wn = None if norm_factor is None else case.win_norm(hard, norm_factor)
        refs = []
        for dt in (torch.float64, torch.float32):
            refs.append([_net_reference(case, n, dt, hard, None if keep is None else keep[n], DROP_P if drop else 0.0, penalty, thres,
                                        None if wn is None else wn[n]) for n in range(case.n_nets)])
        for n, (r64, r32) in enumerate(zip(*refs)):
            hint = (case.id, "net", n, "change the seed (BEH_SEEDS)")
            assert r64["l1_margin"] > KINK_MARGIN, (hint, "a target sits on the L1 kink", r64["l1_margin"])
            live = float(case.mask[n].sum()) > 0
            assert (r64["l1_margin"] < float("inf")) == live, (hint, "the draw masks every target step out")
            assert r64["stab_margin"] > KINK_MARGIN, (hint, "a distance sits on the stability threshold", r64["stab_margin"])
            assert torch.equal(r64["relu"], r32["relu"]), (hint, "fp32 and fp64 take different ReLU branches")
        _REFS[key] = refs
    return _REFS[key]


def launch(case, hard=False, keep=None, seed=0, drop_p=0.0, penalty=0.0, thres=THRES, win_norm=None, accumulate=False, defer=False,
           hist=None, mask=None, E_norm=None):
    """ops.beh_forward + ops.beh_backward (+ the deferred decoder contraction); the hard update runs with the coefficient and
    threshold Behavior_policy.learn of nova/behavior_policy.py passes (1, 0)"""
    dev = case.device
    hist = case.d_hist if hist is None else hist
    fwd = ops.beh_forward(case.enc_arena, case.dec_arena, hist, case.d_mask if mask is None else mask, case.L, case.Z,
                          1.0 if hard else COEF, 0.0 if hard else thres, drop_p, keep=keep, seed=seed, hard=hard, win_norm=win_norm)
    bwd = ops.beh_backward(case.enc_arena, case.dec_arena, fwd, accumulate=accumulate, penalty=penalty,
                           E_norm=hist.shape[1] if E_norm is None else E_norm, defer_dec_wgrad=defer)
    if defer:
        if torch.device(dev).type == "cuda":
            bwd["dec_wgrad"](torch.cuda.Stream(dev))
        else:
            bwd["dec_wgrad"]()
    _sync(dev)
    return fwd, bwd


def _cmp(got, r64, r32, worst, key, what):
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), (what, key, "not finite")
    if float(r64.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, (what, key, "the fp64 reference is exactly zero")
        return
    e32, err = _grad_err(r32, r64), _grad_err(got, r64)
    print(what, key, "err", err, "e32", e32)
    if err >= worst.get(key, -1.0):                            # (the e32 logged beside a worst error is that tensor's own)
        worst[key], worst[key + "_e32"] = err, e32
    _worse(worst, key + "_over_bound", err / _bound(e32))
    assert err <= _bound(e32), (what, key, err, e32)


def compare(case, loss, refs, worst, what, hard=False):
    """both loss components and every parameter's gradient of every net against fp64, each under its own bound"""
    r64, r32 = refs
    loss = loss.detach().double().cpu()
    for n in range(case.n_nets):
        _cmp(loss[n, 0:1], r64[n]["beh"], r32[n]["beh"], worst, "loss", (what, n, "behaviour loss"))
        if not hard:
            _cmp(loss[n, 1:2], r64[n]["stab"], r32[n]["stab"], worst, "loss", (what, n, "stability loss"))
        for name, arena in (("enc", case.enc_arena), ("dec", case.dec_arena)):
            for k in r64[n][name]:
                _cmp(arena.grad_of(n, k), r64[n][name][k], r32[n][name][k], worst, "grad", (what, n, name, k))
    worst["l1_margin"] = min(r["l1_margin"] for r in r64)
    return worst


def _device_keep(case, hard=False):
    return case.keep(hard).to(case.device)


# ------------------------------------------------------------------------------------------------ the restatement itself (CPU only)
def check_restatement():
    """the restated loop equals oracle.behavior_learn_loss and oracle.behavior_hard_learn_loss bit for bit in fp64: both loss values
    and every gradient, with keep flags and a penalty"""
    case = LearnCase(2, 3, 2, 4, 5, 8, 2, "cpu", seed=4)
    for n in range(case.n_nets):
        mine = _net_reference(case, n, torch.float64, keep=case.keep()[n], drop_p=DROP_P, penalty=PENALTY, thres=PENALTY_THRES)
        ep, dp = _req(case.enc_p[n], torch.float64), _req(case.dec_p[n], torch.float64)
        beh, stab, loss = O.behavior_learn_loss(ep, dp, case.view(case.buf)[n].double(), case.mask[n], case.L, COEF, case.keep()[n].double(),
                                                DROP_P, PENALTY, PENALTY_THRES)
        loss.backward()
        assert _bits_equal(mine["beh"], beh.detach().reshape(1)) and _bits_equal(mine["stab"], stab.detach().reshape(1))
        for got, ref in ((mine["enc"], ep), (mine["dec"], dp)):
            assert set(got) == set(ref)
            for k in ref:
                assert _bits_equal(got[k], ref[k].grad), ("soft", n, k)
        mine = _net_reference(case, n, torch.float64, hard=True, keep=case.keep(True)[n], drop_p=DROP_P)
        ep, dp = _req(case.enc_p[n], torch.float64), _req(case.dec_p[n], torch.float64)
        loss = O.behavior_hard_learn_loss(ep, dp, case.view(case.buf)[n].double(), case.mask[n], case.L, case.keep(True)[n].double(), DROP_P)
        loss.backward()
        assert _bits_equal(mine["beh"], loss.detach().reshape(1))
        for got, ref in ((mine["enc"], ep), (mine["dec"], dp)):
            for k in ref:
                assert _bits_equal(got[k], ref[k].grad), ("hard", n, k)


def check_seeded_draw_statistics():
    """from the numpy tensor alone: the keep rate within four binomial standard deviations of 1 - thr / 65536; two seeds differ; the
    threshold is the kernels' ``(uint32_t)(p * 65536.0f)``"""
    shape = (2, 3, 49, 2, 64)
    n = int(np.prod(shape))
    assert keep_threshold(0.1) == 6553 and keep_threshold(0.5) == 32768 and keep_threshold(0.0) == 0
    for p in (0.1, 0.5):
        q = 1.0 - keep_threshold(p) / 65536.0
        for seed in (3, (1 << 40) + 12345):
            k = seeded_keep(seed, p, shape)
            rate, sd = float(k.mean()), (q * (1.0 - q) / n) ** 0.5
            print("p", p, "seed", seed, "keep rate", rate, "expected", q, "sd", sd)
            assert abs(rate - q) <= 4.0 * sd, (p, seed, rate, q, sd)
        assert not np.array_equal(seeded_keep(3, p, shape), seeded_keep(4, p, shape))
        assert not np.array_equal(seeded_keep(3, p, shape), seeded_keep(3 + (1 << 32), p, shape))      # the seed's high word counts
    assert seeded_keep(3, 0.0, shape).all()


# ------------------------------------------------------------------------------------------------ shapes
def check_shape(device, E, N, Lw, J, d, Z, n_nets, env=None, monkeypatch=None):
    """one case against fp64 with drop_p = 0.1 and explicit keep flags (``env``: knobs set for the launch)"""
    case = LearnCase(E, N, Lw, J, d, Z, n_nets, device)
    refs = reference(case, drop=True)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    fwd, _ = launch(case, keep=_device_keep(case), drop_p=DROP_P)
    return compare(case, fwd["loss"], refs, {}, case.id)


def check_mask_kind(device, kind, drops=(False, True)):
    """a mask kind with drop_p = 0 and keep=None, and with drop_p = 0.1 and explicit flags.  "zero_window": a window whose mask sum is
    0 (normaliser 0 + BEPS) adds nothing and nothing non-finite; "zero_net": loss exactly 0, every gradient exactly 0 and finite"""
    case = LearnCase(*MASK_CASE, device, mask_kind=kind)
    worst = {}
    if kind == "zero_window":
        assert float(case.win_norm().min()) == 0.0
    for drop in drops:
        refs = reference(case, drop=drop)
        fwd, _ = launch(case, keep=_device_keep(case) if drop else None, drop_p=DROP_P if drop else 0.0)
        compare(case, fwd["loss"], refs, worst, (case.id, "drop", drop))
        if kind == "zero_net":
            assert float(refs[0][0]["beh"]) == 0.0 and float(fwd["loss"][0, 0]) == 0.0
            for arena in (case.enc_arena, case.dec_arena):
                g = arena.grad[0].cpu()
                assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0, "gradient of an all-masked net"
            assert float(case.enc_arena.grad[1].abs().max()) > 0.0
    return worst


def check_long_episode(device, monkeypatch):
    """513 windows > BEH_D2_MAX_WINDOWS: the decoder forward leaves its second form, and with one BPTT piece asked for beh_backward
    must split the range itself (the second-form BPTT takes at most BEH_D2_MAX_WINDOWS windows per launch)"""
    assert LONG_CASE[3] > L.BEH_D2_MAX_WINDOWS
    monkeypatch.setenv("IPLAN_BEH_PIECES_BWD", "1")
    return check_shape(device, *LONG_CASE)


# ------------------------------------------------------------------------------------------------ forms
def _run_form(device, monkeypatch, rows, form):
    env, opt = FORMS[form]
    opt = dict(opt)
    shards = opt.pop("shards", False)
    case = LearnCase(*(ACC_SHAPES if shards else FORM_SHAPES)[rows], device)
    hard, norm_factor = opt.get("hard", False), opt.pop("norm_factor", None)
    refs = reference(case, hard=hard, drop=True, penalty=opt.get("penalty", 0.0), thres=opt.get("thres", THRES), norm_factor=norm_factor)
    keep = _device_keep(case, hard)
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        if shards:
            # two env shards under the whole batch's window sums: the accumulated arenas hold the whole batch's gradient, the loss
            # shares add up (the stability share of a shard is normalised by its own env count in the forward)
            E, N = case.E, case.N
            wn = ops.beh_window_mask_sums(case.d_mask, case.L)
            cut = E // 2
            loss = torch.zeros(case.n_nets, 2, dtype=torch.float64)
            for c, (lo, hi) in enumerate(((0, cut), (cut, E))):
                fwd, _ = launch(case, keep=keep[:, :, lo * N:hi * N].contiguous(), drop_p=DROP_P, win_norm=wn, accumulate=c > 0,
                                hist=case.d_hist[:, lo:hi], mask=case.d_mask[:, lo:hi].contiguous(), E_norm=E)
                share = fwd["loss"].double().cpu()
                loss[:, 0] += share[:, 0]
                loss[:, 1] += share[:, 1] * (hi - lo) / E
        else:
            wn = None if norm_factor is None else case.win_norm(hard, norm_factor).to(device)
            fwd, _ = launch(case, keep=keep, drop_p=DROP_P, win_norm=wn, **opt)
            loss = fwd["loss"]
    return compare(case, loss, refs, {}, (case.id, form), hard=hard)


def check_form(device, monkeypatch, rows, form):
    """the comparison with fp64 in one launch form at one of the three form shapes"""
    return _run_form(device, monkeypatch, rows, form)


def check_forms_agree(device, monkeypatch, rows):
    """first and second forms differ by less than 3e-6 in worst gradient error, IPLAN_DEC_THIN_ROWS and IPLAN_DEC_BWD_V1 by less
    than 1e-6 (the bounds of test_behavior_learn_decoder_bptt_both_forms_emulated)"""
    w = {f: _run_form(device, monkeypatch, rows, f) for f in ("default", "dec_fwd_v1", "dec_bwd_v1", "dec_thin_rows")}
    g = {f: w[f]["grad"] for f in w}
    print("worst gradient errors", g)
    assert abs(g["dec_thin_rows"] - g["dec_bwd_v1"]) < FORMS_CLOSE_ROWS, g
    assert abs(g["default"] - g["dec_bwd_v1"]) < FORMS_CLOSE_V1_V2, g
    assert abs(g["default"] - g["dec_fwd_v1"]) < FORMS_CLOSE_V1_V2, g
    return {f + "_grad": g[f] for f in g}


# ------------------------------------------------------------------------------------------------ the seeded draw in the kernels
def _results(case, fwd):
    return dict(loss=fwd["loss"].cpu().clone(), saved_lat=fwd["saved_lat"].cpu().clone(), enc_grad=case.enc_arena.grad.cpu().clone(),
                dec_grad=case.dec_arena.grad.cpu().clone())


def _assert_same_bits(a, b, what):
    for k in a:
        assert _bits_equal(a[k], b[k]), (what, k, "differs")


SEEDED_CONFIGS = ((DROP_P, False, (1 << 40) + 12345), (0.5, False, 7), (DROP_P, True, (1 << 33) + 5))     # (drop_p, hard, seed)


def check_seeded_equals_explicit(device, monkeypatch, rows, fwd_v1, bwd_v1, configs=(0, 1, 2), drop0=True):
    """keep=None, seed=s against the same flags recomputed in numpy and passed as ``keep``: loss, both gradient arenas and saved_lat
    bit for bit, in one decoder forward form x one decoder BPTT form -- a seed above 2^32, drop_p 0.1 and 0.5, the hard update
    (``configs``: which of SEEDED_CONFIGS); and the production path end to end: the first configuration's results against fp64
    autograd on that same tensor.  ``drop0``: drop_p = 0 with a seed equals drop_p = 0 without one."""
    case = LearnCase(*FORM_SHAPES[rows], device)
    if fwd_v1:
        monkeypatch.setenv("IPLAN_DEC_FWD_V1", "1")
    if bwd_v1:
        monkeypatch.setenv("IPLAN_DEC_BWD_V1", "1")
    worst = {}
    for p, hard, seed in (SEEDED_CONFIGS[i] for i in configs):
        shape = (case.n_nets, case.windows(hard), case.rows, case.L, 64)
        flags = torch.from_numpy(seeded_keep(seed, p, shape))
        fwd, _ = launch(case, hard=hard, keep=None, seed=seed, drop_p=p)
        seeded = _results(case, fwd)
        loss = fwd["loss"].clone()
        fwd, _ = launch(case, hard=hard, keep=flags.to(device), seed=0, drop_p=p)
        _assert_same_bits(seeded, _results(case, fwd), (case.id, "p", p, "hard", hard, "seed", seed))
        if (p, hard, seed) == SEEDED_CONFIGS[0]:
            key = (case.id, case.seed, "seeded", seed)
            if key not in _REFS:
                refs = [[_net_reference(case, n, dt, keep=flags[n], drop_p=p) for n in range(case.n_nets)] for dt in (torch.float64, torch.float32)]
                assert min(r["l1_margin"] for r in refs[0]) > KINK_MARGIN, (key, "a target sits on the L1 kink: change the seed (BEH_SEEDS)")
                assert all(torch.equal(a["relu"], b["relu"]) for a, b in zip(*refs)), (key, "fp32 and fp64 take different ReLU branches")
                _REFS[key] = refs
            compare(case, loss, _REFS[key], worst, (case.id, "seeded"))     # (the arenas hold the bits of the seeded launch)
    if drop0:
        fwd, _ = launch(case, keep=None, seed=0, drop_p=0.0)
        plain = _results(case, fwd)
        fwd, _ = launch(case, keep=None, seed=(1 << 40) + 12345, drop_p=0.0)
        _assert_same_bits(plain, _results(case, fwd), (case.id, "drop_p = 0 with a seed"))
    return worst


# ------------------------------------------------------------------------------------------------ ownership and repeatability
def check_ownership_and_repeatability(device, monkeypatch, bwd_v1, rows=17, runs=4):
    """both gradient arenas back to back inside one sentinel-filled buffer: beh_backward leaves the guards and the padding between
    the tensors bit-unchanged; pre-filled with NaN (accumulate=False) it leaves no NaN in any parameter's gradient; two identical
    calls give identical bits and the NaN prefill changes none; the strided ``hist`` view gives the bits of a contiguous copy"""
    case = LearnCase(*FORM_SHAPES[rows], device)
    if bwd_v1:
        monkeypatch.setenv("IPLAN_DEC_BWD_V1", "1")
    keep = _device_keep(case)
    arenas = [case.enc_arena, case.dec_arena]
    results = []
    for fill, hist in ((None, None), (float("nan"), None), (None, None), (None, case.d_hist.contiguous()))[:runs]:
        big, init, spans = _rehome_grads(arenas, device, fill)
        fwd, _ = launch(case, keep=keep, drop_p=DROP_P, hist=hist)
        got = big.cpu()
        own = torch.zeros(big.numel(), dtype=torch.bool)
        for (lo, hi), arena in zip(spans, arenas):
            own[lo:hi] = _param_slots(arena).flatten()
        assert not torch.isnan(got[own]).any(), "a parameter's gradient was left unwritten"
        assert _bits_equal(got[~own], init[~own]), "beh_backward wrote outside the parameters' gradient slots"
        results.append(dict(loss=fwd["loss"].cpu().clone(), saved_lat=fwd["saved_lat"].cpu().clone(), grad=got[own]))
    for what, r in zip(("the NaN prefill", "a second call", "a contiguous hist"), results[1:]):
        _assert_same_bits(results[0], r, what)
    return {}


def check_row_independence(device, E=4, N=12, Lw=2, J=3, d=5, Z=8, n_nets=1):
    """dropping the last env (under the same injected window sums) changes no ``saved_lat`` row of the envs that remain and no loss
    numerator share of a tile made of their rows alone (48 -> 36 rows: tiles 0 and 1)"""
    case = LearnCase(E, N, Lw, J, d, Z, n_nets, device)
    keep = _device_keep(case)
    wn = ops.beh_window_mask_sums(case.d_mask, Lw)
    full, _ = launch(case, keep=keep, drop_p=DROP_P, win_norm=wn)
    rows = (E - 1) * N
    part, _ = launch(case, keep=keep[:, :, :rows].contiguous(), drop_p=DROP_P, win_norm=wn, hist=case.d_hist[:, :E - 1],
                     mask=case.d_mask[:, :E - 1].contiguous())
    assert _bits_equal(part["saved_lat"], full["saved_lat"][:, :rows]), "a remaining env's saved_lat rows changed"
    tiles = rows // 16
    assert tiles >= 2 and _bits_equal(part["loss_part"][:, :tiles, 0], full["loss_part"][:, :tiles, 0]), "a remaining tile's loss share changed"
    return {}


# ------------------------------------------------------------------------------------------------ refusals, single-window decoder
class _Recorder:
    """a library stand-in that keeps the argument struct of the last call and passes the call on"""

    def __init__(self):
        self.lib, self.args = ops._lib(None), None

    def call(self, name, a, stream=None):
        self.args = a
        return self.lib.call(name, a, stream)


def _bdec_inputs(device, rows, Lw, d, Z, n_nets, with_keep, seed=0):
    from iplan_amd.arena import ParamArena
    from iplan_amd.nova.behavior_net import Behavior_Latent_Decoder, EncoderRNN
    torch.manual_seed(500 + 10 * rows + d + seed)
    enc = [EncoderRNN(input_size=d, hidden_size=32, output_size=Z, num_layers=1) for _ in range(n_nets)]
    dec = [Behavior_Latent_Decoder(input_size=d + Z, hidden_size=64, output_size=d, num_layers=1, dropout=0.0) for _ in range(n_nets)]
    dec_p = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in dec]
    gen = torch.Generator().manual_seed(seed + rows + d)
    window = torch.rand(n_nets, rows, Lw, d, generator=gen) * 2 - 1
    latent = torch.softmax(torch.randn(n_nets, rows, Z, generator=gen), -1)
    hidden = torch.randn(n_nets, rows, 64, generator=gen) * 0.5
    keep = (torch.rand(n_nets, 1, rows, Lw, 64, generator=gen) < 1.0 - DROP_P).to(torch.uint8) if with_keep else None
    return ParamArena(enc, device), ParamArena(dec, device), dec_p, window, latent, hidden, keep


def check_bdec_forward(device, rows, d, Z, with_keep, Lw=3, n_nets=2):
    """ops.bdec_forward (single-window mode of iplan_beh_fwd: the decoder forward's first form) against fp64
    oracle.decoder_forward: ``pred`` and the new hidden state of every net"""
    enc_arena, dec_arena, dec_p, window, latent, hidden, keep = _bdec_inputs(device, rows, Lw, d, Z, n_nets, with_keep)
    pred, hout = ops.bdec_forward(enc_arena, dec_arena, window.to(device), latent.to(device), hidden.to(device), drop_p=DROP_P if with_keep else 0.0,
                                  keep=None if keep is None else keep.to(device))
    _sync(device)
    assert pred.shape == (n_nets, rows, Lw, d) and hout.shape == (n_nets, rows, 64)
    worst = {}
    for n in range(n_nets):
        ref = {}
        for dt in (torch.float64, torch.float32):
            dp = O.strip_prefix({k: v.to(dt) for k, v in dec_p[n].items()}, "decoder.")
            x = torch.cat([window[n], latent[n][:, None, :].expand(rows, Lw, Z)], -1).to(dt)
            ref[dt] = O.decoder_forward(dp, x, hidden[n].to(dt), None if keep is None else keep[n, 0].to(dt), DROP_P if with_keep else 0.0)
        for key, got, i in (("pred", pred[n], 0), ("hidden", hout[n], 1)):
            _cmp(got, ref[torch.float64][i], ref[torch.float32][i], worst, key, ("bdec", rows, d, Z, with_keep, n))
    return worst


def check_refusals(device, monkeypatch):
    """the entry points' own argument checks, each refusal naming its reason: d + Z > 16, d = 0, J < 1; drop_p = 1; a window range
    without carries; dec_thin_part together with IPLAN_DEC_BWD_V1; the BPTT in single-window mode"""
    lib, stream = ops._lib(None), L.current_stream(device)
    monkeypatch.setenv("IPLAN_BEH_PIECES", "1")                # (one launch each way: no window range, no carries in the struct)
    case = LearnCase(*FORM_SHAPES[17], device)
    fwd, bwd = launch(case)
    a = fwd["_args"]
    assert not a.fwd_phase and not a.bwd_phase and a.dec_thin_part

    def with_fields(entry, needle, **fields):
        old = {k: getattr(a, k) for k in fields}
        for k, v in fields.items():
            setattr(a, k, v)
        _refused(lambda: lib.call(entry, a, stream), needle)
        for k, v in old.items():
            setattr(a, k, v)

    for entry in ("iplan_beh_fwd", "iplan_beh_bwd"):
        with_fields(entry, "unsupported dims", d=12)                            # 12 + 8 > 16
        with_fields(entry, "unsupported dims", d=0)
        with_fields(entry, "unsupported dims", T=a.L + 1)                       # J = 0
        with_fields(entry, "dropout p=", drop_p=1.0)
    with_fields("iplan_beh_fwd", "a window range needs enc_carry", fwd_phase=1, fwd_j_lo=0, fwd_j_hi=1, enc_carry=None, dec_carry=None)
    with_fields("iplan_beh_bwd", "a window range needs bwd_phase", bwd_phase=1, bwd_j_lo=0, bwd_j_hi=1, dec_carry=None)
    with_fields("iplan_beh_bwd", "a window range needs bwd_phase", bwd_phase=2, bwd_j_lo=1, bwd_j_hi=2, enc_carry=None)
    with monkeypatch.context() as mp:
        mp.setenv("IPLAN_DEC_BWD_V1", "1")
        _refused(lambda: lib.call("iplan_beh_bwd", a, stream), "only supported by the decoder BPTT's second form")
    _sync(device)
    before = _results(case, fwd)
    again, _ = launch(case)                                                      # the struct restored: the first run's bits
    _assert_same_bits(before, _results(case, again), "after the refusals")
    del bwd
    rec = _Recorder()
    enc_arena, dec_arena, _, window, latent, hidden, _ = _bdec_inputs(device, 17, 3, 5, 8, 1, False)
    dev_in = [t.to(device) for t in (window, latent, hidden)]
    ops.bdec_forward(enc_arena, dec_arena, *dev_in, lib=rec)
    _sync(device)
    assert rec.args is not None and rec.args.win
    _refused(lambda: lib.call("iplan_beh_bwd", rec.args, stream), "not available in single-window decoder mode")
    return {}
