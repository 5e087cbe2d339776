"""TEST INFRASTRUCTURE: the three kernels of a rollout vector step alone -- enc_fwd_kernel (csrc/behavior.hip, body in csrc/enc_body.h)
through ops.enc_forward, gat_enc_fwd_kernel and gat_enc_ac_fwd_kernel (csrc/gat.hip) through ops.gat_forward(fuse_enc=, fuse_ac=) -- on
whatever library is active: the host emulator in tests/test_emu_rollout_step.py, the gfx950 build in tests/test_gpu_rollout_step.py.

Ground truth and bounds, none of them new:
* the encoder: oracle.latent_update in fp64 and in fp32; error = max|got - ref64| / max|ref64| per tensor and net, bound 1e-5, the fp32
  oracle's own error asserted below 6.7e-6 (tests/kernel_checks.py);
* the scenes: kernel_checks.GatCase.reference at tau = 1 under check_gat_kernels' rule (error relative to max(1, |ref64|), bound 1e-5);
* the action selection: ac_forward_checks' rule and its 1e-4 margin between the two largest keys p / q of the sampled head;
* one launch against the separate launches of the same step: the bits on the emulator, 2e-6 x max(1, |ref|) on the GPU (separate
  instantiations of one source, rollout_oracle.check_rollout_body).
Operands are passed the way the rollout passes them: strided views, in their first two dimensions, of larger buffers -- inputs with NaN
around them, destinations with a sentinel pattern that must survive in every float the launch does not own.
The checks never touch ``L.use_library_for_tests``; each returns the worst errors it saw."""
import ctypes as C
import functools

import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import ac_forward_checks as AC
from tests import policy_trace_checks as PC
from tests import rollout_oracle as RO
from tests.kernel_checks import E32_MAX, GAT_A, TOL, GatCase, _rel1, _sentinel
from tests.oracle_checks import _grad_err
from tests.policy_trace_checks import _bits, _sync, _worse

ER = 32                       # encoder_rnn_dim of the kernels (csrc/enc_body.h)
FUSED_TOL = 2e-6              # one launch against the separate ones on the GPU (rollout_oracle.check_rollout_body)
KEY_MARGIN = 1e-4             # between the two largest keys p / q of a sampled row (ac_forward_checks)
COEF = 0.1                    # soft_update_coef


# ------------------------------------------------------------------------------------------------ operands in place
class Carved:
    """a [n_nets, B, inner] view -- env-major storage [B + 2, n_nets + 1, 4 + inner + 4], i.e. a spare environment either side, a spare
    net and four floats around every innermost block, so both leading strides differ from the packed ones and every block stays 16-byte
    aligned when inner % 4 == 0 -- of a buffer that holds ``values`` inside the view and NaN around it (an input) or the sentinel
    pattern everywhere (a destination)"""

    def __init__(self, n_nets, B, inner, device, values=None):
        shape = (B + 2, n_nets + 1, inner + 8)
        if values is None:
            self.init = _sentinel(shape[0] * shape[1] * shape[2]).view(shape).clone()
        else:
            self.init = torch.full(shape, float("nan"))
            self.init[1:1 + B, :n_nets, 4:4 + inner] = values.reshape(n_nets, B, inner).permute(1, 0, 2)
        self.buf = self.init.clone().to(device)
        self.view = self.buf[1:1 + B, :n_nets, 4:4 + inner].permute(1, 0, 2)
        self.mask = torch.zeros(shape, dtype=torch.bool)
        self.mask[1:1 + B, :n_nets, 4:4 + inner] = True

    def as4(self, N):
        return self.view.unflatten(-1, (N, self.view.shape[-1] // N))

    def assert_owned(self, what):
        """every float outside the view still holds its initial bits, and the view itself was written"""
        host = self.buf.cpu()
        assert torch.equal(_bits(host)[~self.mask], _bits(self.init)[~self.mask]), (what, "a float outside the destination was written")
        assert not torch.equal(_bits(host)[self.mask], _bits(self.init)[self.mask]), (what, "the destination was not written")


def _same(a, b, exact, what, worst=None, key=None):
    """``a`` (one launch) against ``b`` (the separate launches): the bits, or FUSED_TOL x max(1, |b|)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != torch.float32:
        assert torch.equal(a, b), (what, "differ")
        return
    diff = (a.double() - b.double()).abs().max().item() / max(1.0, b.abs().max().item())
    if worst is not None:
        _worse(worst, key, diff)
    if exact:
        assert torch.equal(_bits(a), _bits(b)), (what, "bits differ", diff)
    else:
        assert diff <= FUSED_TOL, (what, diff)


# ------------------------------------------------------------------------------------------------ 1: the encoder alone
# (id, B, N, n_nets, Z, d, L): rows = B N around one wave's tile (16), the standalone workgroup (64) and the fused one (128); N = 1 is
# the encoder's own lower edge (iplan_enc_fwd accepts it, the GAT does not)
ENC_CASES = [
    ("rows1", 1, 1, 1, 8, 5, 3),
    ("rows15_Z1", 3, 5, 2, 1, 5, 3),
    ("rows16_Z3", 2, 8, 2, 3, 5, 3),
    ("rows17_Z4_nets5", 17, 1, 5, 4, 5, 3),
    ("rows63_Z5_d1", 9, 7, 2, 5, 1, 3),
    ("rows64_Z16_d7", 4, 16, 2, 16, 7, 3),
    ("rows65_d16_L1", 5, 13, 2, 8, 16, 1),
    ("rows127_L10", 127, 1, 2, 8, 5, 10),
    ("rows128_Z5_d7", 2, 64, 1, 5, 7, 3),
    ("rows129_nets5", 3, 43, 5, 8, 5, 3),
]


class EncCase:
    """``n_nets`` EncoderRNNs with their own weights in one ParamArena; x is a sliding [t0 : t0 + L] window of a time-major log
    [T, B, n_nets, N, d + 3] permuted to [n_nets, B, N, L, d] (x_s_t is the largest stride, NaN in every float of the log outside the
    window); h0 and prev_latent are Carved inputs"""

    def __init__(self, device, B, N, n_nets=2, Z=8, d=5, Lw=3, seed=0, t0=2):
        from iplan_amd.arena import ParamArena
        from iplan_amd.nova.behavior_net import EncoderRNN
        self.device, self.B, self.N, self.n_nets, self.Z, self.d, self.Lw = device, B, N, n_nets, Z, d, Lw
        base = seed + 7 * B + 1000 * N + 10 * Z + d + 100 * Lw + n_nets
        torch.manual_seed(base)
        self.nets = [EncoderRNN(d, ER, Z, 1) for _ in range(n_nets)]
        gen = torch.Generator().manual_seed(base + 1)
        with torch.no_grad():                  # logits spread over a few units: the default head leaves every latent near uniform
            for m in self.nets:
                m.out.weight.mul_(4.0)
                m.out.bias.add_(torch.randn(Z, generator=gen) * 0.5)
        self.params = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in self.nets]
        self.arena = ParamArena(self.nets, device)
        self.x = torch.rand(n_nets, B, N, Lw, d, generator=gen) * 2 - 1
        self.h0 = torch.randn(n_nets, B, N, ER, generator=gen) * 0.3
        self.prev = torch.softmax(torch.randn(n_nets, B, N, Z, generator=gen), -1)
        log = torch.full((t0 + Lw + 1, B, n_nets, N, d + 3), float("nan"))
        log[t0:t0 + Lw, :, :, :, 1:1 + d] = self.x.permute(3, 1, 0, 2, 4)
        self.log = log.to(device)
        self.d_x = self.log[t0:t0 + Lw, :, :, :, 1:1 + d].permute(2, 1, 3, 0, 4)
        assert self.d_x.shape == self.x.shape and self.d_x.stride(4) == 1 and (Lw == 1 or self.d_x.stride(3) == max(self.d_x.stride()))
        self.c_h0 = Carved(n_nets, B, N * ER, device, self.h0)
        self.c_prev = Carved(n_nets, B, N * Z, device, self.prev)
        self.d_h0, self.d_prev = self.c_h0.as4(N), self.c_prev.as4(N)

    def dests(self):
        """fresh sentinel-filled destinations (latent, hL)"""
        return Carved(self.n_nets, self.B, self.N * self.Z, self.device), Carved(self.n_nets, self.B, self.N * ER, self.device)

    def launch(self, prev, coef, lat, hL, launch=True):
        """ops.enc_forward into the Carved destinations ``lat`` / ``hL`` (or any views of the logical shapes)"""
        lat_v = lat.as4(self.N) if isinstance(lat, Carved) else lat
        hL_v = hL.as4(self.N) if isinstance(hL, Carved) else hL
        res = ops.enc_forward(self.arena, self.d_x, self.d_h0, self.d_prev if prev else None, coef, self.Z, out_lat=lat_v, out_h=hL_v, launch=launch)
        if launch:
            _sync(self.device)
        return res

    def reference(self, dtype, prev, coef):
        """(latent [n_nets, B, N, Z], hL [n_nets, B, N, ER]) in ``dtype`` through oracle.latent_update (computed once, never modified)"""
        return _enc_reference(self, dtype, bool(prev), float(coef))


@functools.lru_cache(maxsize=None)
def _enc_reference(case, dtype, prev, coef):
    ps = [{k: v.to(dtype) for k, v in p.items()} for p in case.params]
    pl = case.prev if prev else torch.zeros_like(case.prev)                           # no previous latent: the softmax itself
    with torch.no_grad():
        lat, hid = O.latent_update(ps, case.x.permute(1, 0, 2, 3, 4).to(dtype), case.h0.permute(1, 0, 2, 3).unsqueeze(1).to(dtype),
                                   pl.permute(1, 0, 2, 3).to(dtype), coef if prev else 1.0)
    return lat.permute(1, 0, 2, 3), hid[:, 0].permute(1, 0, 2, 3)


@functools.lru_cache(maxsize=None)
def get_enc_case(device, B, N, n_nets=2, Z=8, d=5, Lw=3, seed=0):
    return EncCase(device, B, N, n_nets, Z, d, Lw, seed)


def assert_enc_vs_fp64(case, lat, hL, prev, coef, worst, what):
    r64, r32 = case.reference(torch.float64, prev, coef), case.reference(torch.float32, prev, coef)
    for k, got, a, b in (("latent", lat, r64[0], r32[0]), ("hL", hL, r64[1], r32[1])):
        g = got.detach().cpu()
        assert g.shape == a.shape, (what, k, g.shape)
        assert torch.isfinite(g).all(), (what, k, "not finite")
        for n in range(case.n_nets):
            err, e32 = _grad_err(g[n], a[n]), _grad_err(b[n], a[n])
            print(what, k, "net", n, "err", err, "fp32 oracle", e32)
            _worse(worst, k, err)
            _worse(worst, k + "_fp32_oracle_vs_fp64", e32)
            assert e32 < E32_MAX, (what, k, n, "the fp32 oracle's own error: change the case's inputs, not the bound", e32)
            assert err <= TOL, (what, k, n, err)


def check_encoder(device, case):
    """ops.enc_forward of one ENC_CASES entry: without a previous latent (every row on the simplex), with one at coef 0.1, with one at
    coef 1.0 (it drops out: the bits of the launch without), twice into fresh destinations (the same bits); after every launch the
    sentinel around the destinations is intact"""
    what, B, N, n_nets, Z, d, Lw = case
    ec = get_enc_case(device, B, N, n_nets, Z, d, Lw)
    worst = {}
    lat0, hL0 = ec.dests()
    ec.launch(False, 0.0, lat0, hL0)
    assert_enc_vs_fp64(ec, lat0.as4(N), hL0.as4(N), False, 1.0, worst, (what, "no previous latent"))
    p = lat0.as4(N).cpu().double()
    assert (p >= 0).all(), (what, "a negative latent entry")
    off = (p.sum(-1) - 1).abs().max().item()
    _worse(worst, "latent_row_sum", off)
    assert off <= TOL, (what, "a latent row does not sum to 1", off)
    lat1, hL1 = ec.dests()
    ec.launch(False, 0.0, lat1, hL1)
    lat2, hL2 = ec.dests()
    ec.launch(True, COEF, lat2, hL2)
    assert_enc_vs_fp64(ec, lat2.as4(N), hL2.as4(N), True, COEF, worst, (what, "coef", COEF))
    lat3, hL3 = ec.dests()
    ec.launch(True, 1.0, lat3, hL3)
    for tag, (a, b) in (("repeat", (lat1, hL1)), ("coef 1.0", (lat3, hL3))):
        assert torch.equal(_bits(a.view), _bits(lat0.view)), (what, tag, "latent bits differ from the first launch without a previous latent")
        assert torch.equal(_bits(b.view), _bits(hL0.view)), (what, tag, "hL bits differ")
    for c in (lat0, hL0, lat1, hL1, lat2, hL2, lat3, hL3):
        c.assert_owned(what)
    return worst


# ------------------------------------------------------------------------------------------------ 2: scenes + encoder in one launch
# (id, n_nets, (B, N) of the scenes, (B, N) of the encoder, save): the block index maps through n_gat = n_nets B_gat to
# (block - n_gat) / per_net, per_net = (B_enc N_enc + 127) / 128
TWO_WAY_CASES = [
    ("one_block_each_N2", 1, (1, 2), (1, 2), False),
    ("enc128_N16", 2, (2, 16), (8, 16), False),
    ("B_differs_N17", 2, (3, 17), (5, 17), False),
    ("enc128_N64", 2, (2, 64), (2, 64), False),
    ("enc127", 2, (1, 17), (127, 1), False),
    ("enc129_nets5", 5, (1, 3), (3, 43), False),
    ("save_N17", 2, (2, 17), (2, 17), True),
]
GAT_SAVED = ("soft", "hard", "qkv", "x", "h_enc")


def _gat_out_vs_fp64(gc, out, worst, what):
    for n in range(gc.n_nets):
        o64, o32 = gc.reference(n, 1.0, torch.float64)[0], gc.reference(n, 1.0, torch.float32)[0]
        err, e32 = _rel1(out[n].reshape(gc.B * gc.N, GAT_A), o64), _rel1(o32, o64)
        print(what, "out net", n, "err", err, "fp32 oracle", e32)
        _worse(worst, "out", err)
        _worse(worst, "out_fp32_oracle_vs_fp64", e32)
        assert err <= TOL, (what, "out", n, err)


def check_two_way(device, case, exact):
    """ops.gat_forward(fuse_enc=ops.enc_forward(..., launch=False)): out, latent and hL against fp64 by the rules of their standalone
    checks (tau = 1), and against the two separate launches on the same inputs; the sentinel around all three destinations"""
    what, n_nets, (Bg, Ng), (Be, Ne), save = case
    gc = GatCase(device, Bg, Ng, 5, 8, n_nets, strided=True, seed=2)
    ec = get_enc_case(device, Be, Ne, n_nets, 8, 5, 3, seed=1)
    worst = {}
    runs = []
    for fused in (True, False):
        (lat, hL), out = ec.dests(), Carved(n_nets, Bg, Ng * GAT_A, device)
        gat = dict(tau=1.0, save=save, out=out.as4(Ng))
        if fused:
            _, _, enc = ec.launch(True, COEF, lat, hL, launch=False)
            _, saved = ops.gat_forward(gc.arena, gc.d_src0, gc.d_src1, gc.d_h, gc.d_noise, fuse_enc=enc, **gat)
        else:
            _, saved = ops.gat_forward(gc.arena, gc.d_src0, gc.d_src1, gc.d_h, gc.d_noise, **gat)
            ec.launch(True, COEF, lat, hL)
        _sync(device)
        assert (saved is not None) == save
        runs.append((out, lat, hL, saved))
    out, lat, hL, saved = runs[0]
    assert torch.isfinite(out.view).all(), (what, "out is not finite")
    _gat_out_vs_fp64(gc, out.as4(Ng), worst, what)
    assert_enc_vs_fp64(ec, lat.as4(Ne), hL.as4(Ne), True, COEF, worst, what)
    for k, a, b in zip(("out", "latent", "hL"), runs[0][:3], runs[1][:3]):
        _same(a.view, b.view, exact, (what, k, "one launch against two"), worst, k + "_vs_two_launches")
    if save:
        for k in GAT_SAVED:
            _same(saved[k], runs[1][3][k], exact, (what, "saved", k, "one launch against two"), worst, k + "_vs_two_launches")
    for run in runs:
        for c in run[:3]:
            c.assert_owned(what)
    return worst


# ------------------------------------------------------------------------------------------------ 3a: the rollout body at edge shapes
# (n_agents, E, N, other dims, T, seed): the seed leaves every (step, agent, env) outside KEY_MARGIN (body_key_margin, from the oracle's
# rollout alone, on the CPU)
BODY_CASES = [
    (2, 1, 2, {}, 3, 5),                                                   # one row, smallest scene, smallest F
    (2, 15, 3, {}, 3, 5),                                                  # one partial row tile
    (2, 16, 8, {}, 3, 5),                                                  # 128 encoder rows: exactly one fused block
    (2, 17, 17, {}, 2, 5),                                                 # ragged row tile; N one past a scene tile
    (3, 3, 43, {}, 2, 5),                                                  # 129 encoder rows
    (2, 2, 64, {}, 2, 5),                                                  # 128 rows, largest scene
    (2, 2, 63, {}, 2, 5),                                                  # 126 rows
    (3, 100, 3, {}, 2, 5),                                                 # 42 units: the launch picks ksplit_wg = 2 itself; ragged tile
    (2, 5, 6, dict(obs_shape_single=7, latent_dim=5, n_actions=4), 3, 5),  # every w % 4 != 0: non-contiguous k-tiles
    (2, 5, 6, dict(obs_shape_single=3, latent_dim=3), 3, 5),
    (2, 33, 16, dict(latent_dim=4), 2, 5),
]
STALE_CASES = [
    (2, 17, 6, dict(obs_shape_single=7, latent_dim=5), 3, 5),
    (2, 16, 8, {}, 3, 5),
]
KW2_CASE = BODY_CASES[7]


def body_case_id(case):
    nA, E, N, kw, T, seed = case
    return f"nA{nA}_E{E}_N{N}" + "".join(f"_{k}{v}" for k, v in sorted(kw.items()))


def body_args(case, device):
    from iplan_amd.config import default_args
    nA, E, N, kw, T, seed = case
    return default_args("highway", use_cuda=torch.device(device).type == "cuda", max_vehicle_num=N, n_agents=nA, episode_limit=T,
                        batch_size_run=E, max_history_len=3, **kw)


def body_draws(args, E, seed, episode=0):
    """(gumbel noise [T + 1, nA, E, N, N - 1, 2], q_all [T, nA, E, n_actions]) -- episode 0: check_rollout_body's own draws"""
    T, nA, N = args.episode_limit, args.n_agents, args.max_vehicle_num
    gen = torch.Generator().manual_seed(seed + 11 + 1000 * episode)
    u = torch.rand(T + 1, nA, E, N, N - 1, 2, generator=gen).clamp_min(1e-20)
    noise = -torch.log((-torch.log(u)).clamp_min(1e-20))
    q_all = -torch.log(torch.rand(T, nA, E, args.n_actions, generator=gen).clamp_min(1e-20))
    return noise, q_all


def check_body(device, case):
    """rollout_oracle.check_rollout_body, unchanged, at one BODY_CASES entry"""
    return RO.check_rollout_body(body_args(case, device), case[1], device, seed=case[5])


def body_key_margin(case, episodes=(0,)):
    """the smallest relative margin between the two largest keys p / q over every (step, agent, env) of the case's episodes, from the
    fp32 oracle's rollout alone (CPU): bit-equal actions are a condition on the draw, and this is the condition"""
    from iplan_amd.harness import SyntheticLoop
    nA, E, N, kw, T, seed = case
    args = body_args(case, "cpu")
    loop = SyntheticLoop(args, E, seed=seed, device="cpu")
    worst = float("inf")
    for ep in episodes:
        noise, q_all = body_draws(args, E, seed, ep)
        seen, plain = [], O.actor_logits

        def recording(*a, **k):
            res = plain(*a, **k)
            seen.append(res[0])
            return res
        O.actor_logits = recording
        try:
            RO.oracle_rollout(loop, loop.obs_sets[ep], noise, q_all)
        finally:
            O.actor_logits = plain
        assert len(seen) == T * nA
        for j, logits in enumerate(seen):
            keys = torch.softmax(logits.double(), -1) / q_all[j // nA, j % nA].double()
            top = keys.topk(2, -1).values
            worst = min(worst, ((top[:, 0] - top[:, 1]) / top[:, 0]).min().item())
    return worst


def check_launch_picks_kw2(device, mp):
    """the (3, 100, 3) case: 7 row tiles x 3 nets x 2 = 42 units, and ops.ac_forward, left alone, splits each over 2 workgroups"""
    from iplan_amd.harness import SyntheticLoop
    mp.delenv("IPLAN_AC_KSPLIT_WG", raising=False)
    nA, E, N, kw, T, seed = KW2_CASE
    loop = SyntheticLoop(body_args(KW2_CASE, device), E, seed=seed, device=device)
    o = loop.mac.select_actions_ippo(loop.new_batch(), 1, test_mode=False, as_numpy=False, write_back=True, launch=False)
    assert ((E + 15) // 16) * nA * 2 == 42 and o["_args"].ksplit_wg == 2, o["_args"].ksplit_wg
    return {}


# ------------------------------------------------------------------------------------------------ 3b: stale latents must show
CARRIED = ("attention_latent", "behavior_latent", "rnn_states_actors", "rnn_states_critics")


def _assert_counters_zero(what):
    assert ops._FUSED_SYNC and ops._KSPLIT_BUFS, (what, "no fused launch with a K split has run: nothing to read", len(ops._FUSED_SYNC), len(ops._KSPLIT_BUFS))
    for key, b in ops._FUSED_SYNC.items():
        assert b[:3].cpu().tolist() == [0, 0, 0], (what, "sync counters of the fused launch", key, b.cpu().tolist())
    for key, (_, count) in ops._KSPLIT_BUFS.items():
        assert int(count.abs().sum()) == 0, (what, "a k-split ticket counter was left non-zero", key)


def check_stale_latents(device, case, tol=TOL):
    """rollout_oracle.check_rollout_body's driver into ONE container: steps 1 .. T of the carried fields pre-filled with NaN, an episode,
    then -- the batch untouched -- a second episode on the loop's other observation set with new draws.  Both against the oracle of
    their episode: a consumer that read a latent before its producer wrote it finds NaN the first time and the previous episode's
    finite, plausible value the second"""
    from iplan_amd.harness import SyntheticLoop
    nA, E, N, kw, T, seed = case
    args = body_args(case, device)
    loop = SyntheticLoop(args, E, seed=seed, device=device)
    batch = loop.new_batch()
    for k in CARRIED:
        batch.data[k][:, 1:] = float("nan")
    worst = {}
    for ep in (0, 1):
        noise, q_all = body_draws(args, E, seed, ep)
        obs = loop.obs_sets[ep]
        with torch.no_grad():
            loop._rollout_body(obs, batch, noise=noise.to(device), q_all=q_all.to(device))
        _sync(device)
        assert not ops.fused_sync_error(), (ep, "a fused rollout launch gave up waiting for its latent updates")
        _assert_counters_zero((body_case_id(case), "episode", ep))
        ref = RO.oracle_rollout(loop, obs, noise, q_all)
        got = {k: batch.data[k].cpu() for k in ("history",) + CARRIED + ("actions", "actions_onehot")}
        for k in ("history",) + CARRIED:
            assert torch.isfinite(got[k]).all(), (ep, k, "not finite")
        assert torch.equal(got["actions"][:, :T], ref["actions"][:, :T]), (ep, "actions differ")
        assert torch.equal(got["actions_onehot"][:, :T], ref["actions_onehot"][:, :T]), (ep, "one-hots differ")
        for k in ("history",) + CARRIED:
            for t in range(T + 1):
                e = (got[k][:, t].double() - ref[k][:, t].double()).abs().max().item() / max(1.0, ref[k][:, t].abs().max().item())
                _worse(worst, f"episode{ep}_{k}", e)
                assert e < tol, (ep, k, t, e)
    return worst


# ------------------------------------------------------------------------------------------------ 3c: one fused launch from ops pieces
STEP_ROWS = (1, 17, 33)
# seeds of the Exp(1) draws, chosen on the CPU from the fp64 reference's margins alone (pick_step_q_seed)
STEP_Q_SEEDS = {1: 0, 17: 0, 33: 0}


class StepCase(AC.AcCase):
    """an AcCase of ``rows`` environments x one step (k-map edge: latent_dim 6, so N w ends in padded k-tiles for the history and the
    behaviour latent) whose attention_latent and behavior_latent sources are the very tensors a GatCase scene set's ``out`` and an
    EncCase's ``out_lat`` point to.  The CPU masters hold the fp64 latents of the step (what the reference reads); on the device the
    two blocks are NaN until a launch writes them."""
    PAD = 4                                                     # the scenes' ``out`` has to be 16-byte aligned
    LATENT, N_ENT, D = 6, 3, 5

    def __init__(self, rows, device, seed=0):
        self.ready = False
        nA, N, d = 2, self.N_ENT, self.D
        super().__init__((nA, rows, 1, N, d, 5), device, seed=seed, latent=self.LATENT)
        self.gat = GatCase(device, rows, N, d, self.LATENT, nA, strided=True, seed=seed + 1)
        self.enc = EncCase(device, rows, N, nA, self.LATENT, d, 3, seed=seed + 1)
        att = torch.stack([self.gat.reference(n, 1.0, torch.float64)[0].reshape(rows, N * GAT_A) for n in range(nA)])
        lat = self.enc.reference(torch.float64, True, COEF)[0].flatten(2)
        self.latents64 = dict(att=att, beh=lat)                                     # [nA, rows, N w]
        for key, w, t in (("att", GAT_A, att), ("beh", self.LATENT, lat)):
            wide = torch.full((rows, 2, nA, N * w + 8), 0.25, dtype=torch.float64)     # (row stride % 4 == 0)
            wide[:, 0, :, self.PAD:self.PAD + N * w] = t.permute(1, 0, 2)
            self.buf[key] = wide
        self.ready = True
        self.upload()

    def upload(self, order=None):
        super().upload(order)
        if self.ready:
            N = self.N_ENT
            for key, w in (("att", GAT_A), ("beh", self.LATENT)):
                t = self.dbuf[key].float()
                t[:, 0, :, self.PAD:self.PAD + N * w] = float("nan")
                self.dbuf[key] = t

    def latent_view(self, key):
        """[nA, rows, N, w]: the destination of the producer AND (AcCase.spec) the source of the action selection"""
        N, w = self.N_ENT, GAT_A if key == "att" else self.LATENT
        return self.dbuf[key][:, 0, :, self.PAD:self.PAD + N * w].unflatten(-1, (N, w)).permute(1, 0, 2, 3)

    def q(self):
        return AC._q_noise(self, STEP_Q_SEEDS[self.rows])

    def step(self, mp, fused, q, count=None):
        """the step into fresh (NaN) latent blocks: one launch, or the three separate ones in stream order.  Returns (the action
        selection's outputs, attention latent, behaviour latent, the encoder's hL destination)"""
        self.upload()
        gc, ec = self.gat, self.enc
        att, beh, hL = self.latent_view("att"), self.latent_view("beh"), Carved(ec.n_nets, ec.B, ec.N * ER, self.device)
        assert att.data_ptr() == self.spec().sources[1][0].data_ptr() and beh.data_ptr() == self.spec().sources[2][0].data_ptr()
        scene = (gc.arena, gc.d_src0, gc.d_src1, gc.d_h, gc.d_noise)
        if fused:
            ac = self.run("rollout_kw4", mp, mode=1, q=q, dest=dict(launch=False))
            _, _, enc = ec.launch(True, COEF, beh, hL, launch=False)
            n0 = count() if count else 0
            ops.gat_forward(*scene, tau=1.0, out=att, fuse_enc=enc, fuse_ac=ac)
            self.fused_blocks = count() - n0 if count else None                  # (check_grids: the emulator's view of the grid)
            _sync(self.device)
            assert not ops.fused_sync_error(), "the fused launch gave up waiting for its latent updates"
            _assert_counters_zero(("step", self.rows))
        else:
            ops.gat_forward(*scene, tau=1.0, out=att)
            ec.launch(True, COEF, beh, hL)
            ac = self.run("rollout_kw4", mp, mode=1, q=q)
        return ac, att.clone(), beh.clone(), hL


@functools.lru_cache(maxsize=None)
def get_step_case(rows, device):
    return StepCase(rows, device)


def pick_step_q_seed(rows, tries=50):
    """the first seed whose Exp(1) draw leaves no row of the case inside KEY_MARGIN, from the fp64 reference alone (CPU)"""
    case = get_step_case(rows, "cpu")
    for seed in range(tries):
        if bool(AC._sample_margin(case, AC._q_noise(case, seed))[1].all()):
            return seed
    raise AssertionError("no seed found")


STEP_OUTS = ("logp", "entropy", "probs", "values", "h_actor", "h_critic")


def check_step(device, mp, rows, exact):
    """one iplan_gat_enc_ac_fwd launch built from ops pieces (which = 2, sampled head, K split over 4 workgroups): (i) its action
    selection against the fp64 oracle on the fp64 latents of the same step under ac_forward_checks' rule, the sampled action == the
    fp64 argmax of p / q (no row inside the margin at the committed seed), the latents it wrote against fp64; (ii) everything against
    the three separate launches in stream order"""
    case = get_step_case(rows, device)
    what = ("step", rows)
    q = case.q()
    keys, clear = AC._sample_margin(case, q)
    assert bool(clear.all()), (what, "rows inside the margin at the committed seed", int((~clear).sum()))
    qd = q.to(device).contiguous()
    got, att, beh, hL = case.step(mp, True, qd)
    worst = {}
    for k in STEP_OUTS:
        assert torch.isfinite(got[k]).all(), (what, k, "not finite")
    assert torch.isfinite(att).all() and torch.isfinite(beh).all(), (what, "a latent block was left unwritten")
    AC.assert_vs_fp64(case, got, worst, what, [k for k in STEP_OUTS if k != "logp"])
    AC.assert_head_edges(case, got, what, mode2=False)
    acts = got["actions"].cpu()
    assert torch.equal(acts, keys.argmax(-1)), (what, "sampled action differs from the fp64 argmax of p / q")
    for i in range(acts.shape[0]):             # logp of the action the launch drew (the reference's own is of the recorded one)
        lp64, lp32 = (case.reference(dt)["probs"][i].log().gather(-1, acts[i].unsqueeze(-1))[:, 0] for dt in (torch.float64, torch.float32))
        err, e32 = _grad_err(got["logp"][i], lp64), _grad_err(lp32, lp64)
        _worse(worst, "logp", err)
        _worse(worst, "logp_e32", e32)
        assert err <= PC._bound(e32), (what, "logp", i, err, e32)
    for key, t in (("att", att), ("beh", beh)):
        for n in range(t.shape[0]):
            ref = case.latents64[key][n]
            err = _rel1(t[n].flatten(1), ref) if key == "att" else _grad_err(t[n].flatten(1), ref)
            _worse(worst, key, err)
            assert err <= TOL, (what, key, n, err)
    hL.assert_owned(what)
    # the standalone action selection on the very latents the fused launch wrote (recorded: what of the difference below is the two
    # instantiations of ac_fwd_body alone, what the last bits of the latents fed through LayerNorm(F), fc1 and the GRU)
    same = case.run("rollout_kw4", mp, mode=1, q=qd)
    for k in STEP_OUTS:
        _same(got[k], same[k], exact, (what, k, "fused against the standalone action selection on the same latents"), worst, k + "_vs_ac_alone_same_latents")
    sep, att2, beh2, hL2 = case.step(mp, False, qd)
    assert torch.equal(acts, sep["actions"].cpu()), (what, "actions differ from the three separate launches")
    for k in STEP_OUTS:
        _same(got[k], sep[k], exact, (what, k, "one launch against three"), worst, k + "_vs_three_launches")
    for k, a, b in (("att", att, att2), ("beh", beh, beh2), ("hL", hL.view, hL2.view)):
        _same(a, b, exact, (what, k, "one launch against three"), worst, k + "_vs_three_launches")
    return worst


# ------------------------------------------------------------------------------------------------ the grids (emulator only)
def check_grids(device, mp, blocks_launched):
    """``blocks_launched``: the emulator's count of workgroups launched so far -- the hardware has no such view.  The grids restated:
    64 encoder rows per workgroup standalone, 128 in the fused launches behind n_nets x B scenes, and (rows + 15) / 16 x ksplit_wg x
    n_agents x 2 action-selection workgroups last.  A grid that is too large computes the same thing on idle workgroups: no output shows it"""
    for what, n_nets, (Bg, Ng), (Be, Ne), save in TWO_WAY_CASES:
        gc = GatCase(device, Bg, Ng, 5, 8, n_nets, strided=True, seed=2)
        ec = get_enc_case(device, Be, Ne, n_nets, 8, 5, 3, seed=1)
        (lat, hL), out = ec.dests(), Carved(n_nets, Bg, Ng * GAT_A, device)
        n0 = blocks_launched()
        ec.launch(True, COEF, lat, hL)
        n1 = blocks_launched()
        assert n1 - n0 == n_nets * ((Be * Ne + 63) // 64), (what, "iplan_enc_fwd", n1 - n0)
        _, _, enc = ec.launch(True, COEF, lat, hL, launch=False)
        ops.gat_forward(gc.arena, gc.d_src0, gc.d_src1, gc.d_h, gc.d_noise, tau=1.0, save=save, out=out.as4(Ng), fuse_enc=enc)
        n2 = blocks_launched()
        assert n2 - n1 == n_nets * Bg + n_nets * ((Be * Ne + 127) // 128), (what, "iplan_gat_enc_fwd", n2 - n1)
    for rows in STEP_ROWS:
        case = get_step_case(rows, device)
        nA, N = case.dims[0], case.N_ENT
        qd = case.q().to(device).contiguous()
        case.step(mp, True, qd, count=blocks_launched)
        want = nA * rows + nA * ((rows * N + 127) // 128) + ((rows + 15) // 16) * 4 * nA * 2
        assert case.fused_blocks == want, (rows, "iplan_gat_enc_ac_fwd", case.fused_blocks, want)
    return {}


# ------------------------------------------------------------------------------------------------ 4: refusals
ENC_DIMS_BAD = [dict(d=0), dict(d=17), dict(Z=0), dict(Z=17), dict(L=0), dict(n_nets=0)]
ENC_NULL_BAD = [dict(x=None), dict(h0=None), dict(hL=None), dict(latent_out=None), dict(params=None)]
ENTRIES = ("iplan_enc_fwd", "iplan_gat_enc_fwd", "iplan_gat_enc_ac_fwd")
# the message of the check each refusal is meant to reach, per entry point (csrc/behavior.hip, csrc/gat.hip, csrc/actor_critic.hip)
WHY = {
    "dims": dict(zip(ENTRIES, ("unsupported dims", "unsupported encoder dims", "unsupported encoder dims"))),
    "null": dict(zip(ENTRIES, ("null tensor pointer", "null encoder tensor pointer", "null encoder tensor pointer"))),
    "null_e": dict(zip(ENTRIES, ("null args", "null encoder args", "null encoder / actor-critic args or sync"))),
}


def check_refusals(device, mp):
    """the argument checks of the three entry points, which return before any launch: non-zero, a message that names the entry point
    AND the check the call is meant to reach, every destination as it was, the sync counters untouched; afterwards the restored
    descriptors launch.  The action-selection part is refused twice over: from a descriptor with ksplit_wg = 0 (form ``rollout``), which
    passes the checks shared with iplan_ac_fwd so that the three-way entry's own rule ("rollout-shaped") is what refuses, and from the
    ksplit_wg = 4 descriptor, where the shared rule refuses first -- under the three-way entry's name"""
    case = get_step_case(17, device)
    lib = ops._lib(None)
    stream = C.c_void_p(L.current_stream(torch.device(device)) or 0)
    qd = case.q().to(device).contiguous()
    case.upload()
    gc, ec = case.gat, case.enc
    att, beh, hL = case.latent_view("att"), case.latent_view("beh"), Carved(ec.n_nets, ec.B, ec.N * ER, device)
    _, saved = ops.gat_forward(gc.arena, gc.d_src0, gc.d_src1, gc.d_h, gc.d_noise, tau=1.0, save=True, out=att)      # a valid launch: its descriptor
    a = saved["_args"]
    for k in ("h_enc", "gru", "qkv", "soft", "hard", "x", "cell"):                                                     # (the rollout's form saves nothing)
        setattr(a.saved, k, None)
    _, _, enc = ec.launch(True, COEF, beh, hL, launch=False)
    e = enc["args"]
    ac = case.run("rollout_kw4", mp, mode=1, q=qd, dest=dict(launch=False))
    ac0 = case.run("rollout", mp, mode=1, q=qd, dest=dict(launch=False))
    c, c0 = ac["_args"], ac0["_args"]
    assert c.ksplit_wg == 4 and c0.ksplit_wg == 0
    sync = torch.tensor([0, 0, 0, 12345], dtype=torch.int32, device=device)
    scratch = torch.zeros(64, device=device)
    assert scratch.data_ptr() % 16 == 0
    dests = [case.dbuf["att"], case.dbuf["beh"], hL.buf] + [ac[k] for k in STEP_OUTS] + [ac0[k] for k in STEP_OUTS]
    for t in dests:
        t.fill_(7.5)
    ac["actions"].fill_(77)
    ac0["actions"].fill_(77)
    _sync(device)
    count = 0

    def call(entry, null_e=False, null_sync=False, cc=None):
        pe = None if null_e else C.byref(e)
        if entry == "iplan_enc_fwd":
            return lib.c.iplan_enc_fwd(pe, stream)
        if entry == "iplan_gat_enc_fwd":
            return lib.c.iplan_gat_enc_fwd(C.byref(a), pe, stream)
        return lib.c.iplan_gat_enc_ac_fwd(C.byref(a), pe, C.byref(c if cc is None else cc), None if null_sync else C.c_void_p(sync.data_ptr()), stream)

    def refused(entry, why, obj=None, fields=None, **kw):
        nonlocal count
        keep = {k: getattr(obj, k) for k in (fields or {})}
        for k, v in (fields or {}).items():
            setattr(obj, k, v)
        try:
            rc = call(entry, **kw)
            msg = lib.c.iplan_last_error().decode()
        finally:
            for k, v in keep.items():
                setattr(obj, k, v)
        assert rc != 0 and msg.startswith(entry + ":") and why in msg, (entry, why, fields, sorted(kw), rc, msg)
        count += 1

    for entry in ENTRIES:
        for fields in ENC_DIMS_BAD:
            refused(entry, WHY["dims"][entry], e, fields)
        for fields in ENC_NULL_BAD:
            refused(entry, WHY["null"][entry], e, fields)
        refused(entry, WHY["null_e"][entry], null_e=True)
    for entry in ENTRIES[1:]:
        for N in (1, 65):
            refused(entry, f"N={N} outside [2,", a, dict(N=N))
        refused(entry, "16-byte aligned", a, dict(out=a.out + 4))
    refused(ENTRIES[2], WHY["null_e"][ENTRIES[2]], null_sync=True)
    # the three-way entry's own rule (ksplit != 8 || saved || fc1_pre || ln_stats_mode != 0): the ksplit_wg = 0 descriptor with one field
    # off passes ac_fwd_check; fc1_pre passes it only beside ksplit 1 and stored statistics, alone the shared rule refuses it
    fc1 = dict(fc1_pre=scratch.data_ptr(), ksplit=1, ln_stats_mode=2, ln_stats=scratch.data_ptr())
    for fields in (dict(ksplit=1), dict(saved=scratch.data_ptr()), dict(ln_stats_mode=1), fc1):
        refused(ENTRIES[2], "rollout-shaped", c0, fields, cc=c0)
    refused(ENTRIES[2], "fc1_pre needs", c0, dict(fc1_pre=scratch.data_ptr()), cc=c0)
    # ... and from the ksplit_wg = 4 descriptor the checks shared with iplan_ac_fwd refuse first, in this entry's name
    for fields in (dict(ksplit=1), dict(saved=scratch.data_ptr()), dict(ln_stats_mode=1)):
        refused(ENTRIES[2], "ksplit_wg needs", c, fields)
    refused(ENTRIES[2], "fc1_pre needs", c, dict(fc1_pre=scratch.data_ptr()))
    _sync(device)
    for t in dests:
        assert bool((t == 7.5).all()), "a refused call wrote a destination"
    assert bool((ac["actions"] == 77).all()) and bool((ac0["actions"] == 77).all()), "a refused call wrote the actions"
    assert sync.cpu().tolist() == [0, 0, 0, 12345], ("a refused call touched the sync counters", sync.cpu().tolist())
    # the same descriptors, every field restored, are accepted
    assert call(ENTRIES[2]) == 0, lib.c.iplan_last_error().decode()
    _sync(device)
    assert sync.cpu().tolist() == [0, 0, 0, 12345]
    for k in STEP_OUTS:
        assert torch.isfinite(ac[k]).all(), (k, "the restored descriptors did not run")
    return {"refused": float(count)}
