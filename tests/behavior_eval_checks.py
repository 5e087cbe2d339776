"""TEST INFRASTRUCTURE: behaviour-model inference (csrc/behavior_eval.hip, ops.beh_eval, Behavior_policy.evaluate / latent_trace) on
whatever library is active -- the host emulator in tests/test_emu_behavior_eval.py, the gfx950 build in
tests/test_gpu_behavior_eval.py.

References: the loop of oracle.behavior_learn_loss with drop_masks=None, restated here window by window from
oracle.behavior_windows / decoder_forward / encoder_forward so that the per-window latents, reconstructions and per-(j, t) sums
are visible, in fp64 and fp32 (``check_policy_methods`` checks the restatement against oracle.behavior_learn_loss itself).
Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor (``_grad_err``), bound = max(1e-5, E32_FACTOR x the
fp32 reference's own error against fp64), the fp32 error computed beside every fp64 reference.
The checks never touch ``L.use_library_for_tests``: the caller decides which library is active.  Each returns the worst errors it saw."""
import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5

# (E, N, L, J, d, Z, n_nets): rows E * N in {2, 15, 16, 17, 65} -- below, at and one past a wave's 16 rows, more than one workgroup
# (65 rows = 5 tiles) --; L in {1, 2, 10}; J in {1, 2, L - 1, L + 3} -- curr fully padded, partly padded and unpadded --; every
# (d, Z) with the latent starting inside a lane group (d = 5), at its edge (4, 8, 12) and filling the tile (8 + 8, 12 + 4)
KERNEL_CASES = [
    (1, 2, 1, 1, 4, 1, 1), (1, 2, 10, 13, 5, 8, 5), (3, 5, 2, 1, 8, 8, 1), (3, 5, 10, 9, 12, 4, 5), (2, 8, 1, 4, 5, 8, 5),
    (2, 8, 10, 2, 4, 1, 1), (1, 17, 2, 5, 12, 4, 1), (1, 17, 10, 1, 8, 8, 5), (5, 13, 2, 2, 5, 8, 5), (5, 13, 10, 13, 4, 1, 1),
    (5, 13, 1, 2, 12, 4, 1), (3, 5, 2, 5, 5, 8, 1),
]
COEF, THRES = 0.1, 0.005


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


class Case:
    """random encoder / decoder parameters and an episode buffer [E, T, net, N * d] whose env, step and net strides are all
    larger than the packed ones, handed to the kernel as the permuted view [net, E, T, N, d] that ``prepare_learn`` produces;
    0/1 masks with zeros in the middle of every episode"""

    def __init__(self, E, N, Lw, J, d, Z, n_nets, device, seed=0, dropout=0.0):
        from iplan_amd.arena import ParamArena
        from iplan_amd.nova.behavior_net import Behavior_Latent_Decoder, EncoderRNN
        self.E, self.N, self.L, self.J, self.d, self.Z, self.n_nets, self.device = E, N, Lw, J, d, Z, n_nets, device
        self.T = T = J + 1 + Lw
        torch.manual_seed(10000 * E + 1000 * N + 100 * Lw + 10 * J + d + Z + n_nets + seed)
        self.enc = [EncoderRNN(input_size=d, hidden_size=32, output_size=Z, num_layers=1) for _ in range(n_nets)]
        self.dec = [Behavior_Latent_Decoder(input_size=d + Z, hidden_size=64, output_size=d, num_layers=1, dropout=dropout) for _ in range(n_nets)]
        self.enc_p = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.enc]
        self.dec_p = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in self.dec]
        self.enc_arena, self.dec_arena = ParamArena(self.enc, device), ParamArena(self.dec, device)
        gen = torch.Generator().manual_seed(seed + E + N + Lw + J + d)
        self.buf = torch.rand(E, T + 2, n_nets + 1, N * d + 3, generator=gen) * 2 - 1
        self.mask = (torch.rand(n_nets, E, T, generator=gen) < 0.7).float()
        self.mask[:, :, T // 2] = 0.0                                      # a zero mid-episode in every env
        self.mask[:, 0, -1] = 1.0                                          # ... and something that counts
        self.upload()

    def view(self, buf):
        E, T, n, N, d = self.E, self.T, self.n_nets, self.N, self.d
        return buf[:, 1:T + 1, :n, :N * d].unflatten(-1, (N, d)).permute(2, 0, 1, 3, 4)        # [net, E, T, N, d]

    def upload(self):
        self.d_buf, self.d_mask = self.buf.to(self.device), self.mask.to(self.device).contiguous()
        self.d_hist = self.view(self.d_buf)
        assert not self.d_hist.is_contiguous() and self.d_hist.stride(3) == self.d

    def run(self, latent=True, recon=True, sums=True):
        out = ops.beh_eval(self.enc_arena, self.dec_arena, self.d_hist, self.d_mask if sums else None, self.L, self.Z, COEF, THRES,
                           want_latent=latent, want_recon=recon, want_sums=sums)
        _sync(self.device)
        return out

    def reference(self, dtype):
        """(latent [n, rows, J, Z], recon [n, rows, J, L, d], sums [n, J, L, 2]) in ``dtype``: the loop of
        oracle.behavior_learn_loss, drop_masks=None, with its per-window values kept"""
        E, N, Lw, J, d, Z = self.E, self.N, self.L, self.J, self.d, self.Z
        hist = self.view(self.buf).to(dtype)
        lats, recs, sums = [], [], []
        for n in range(self.n_nets):
            ep = {k: v.to(dtype) for k, v in self.enc_p[n].items()}
            dp = O.strip_prefix({k: v.to(dtype) for k, v in self.dec_p[n].items()}, "decoder.")
            latent = torch.zeros(E, N, Z, dtype=dtype)
            eh, dh = torch.zeros(E * N, 32, dtype=dtype), torch.zeros(E * N, 64, dtype=dtype)
            lat_j, rec_j, s = [], [], torch.zeros(J, Lw, 2, dtype=dtype)
            for j in range(J):
                curr, nxt, mn = O.behavior_windows(hist[n], self.mask[n], j, Lw)
                dec_in = torch.cat([curr, latent[:, :, None, :].expand(E, N, Lw, Z)], dim=-1)
                pred, dh = O.decoder_forward(dp, dec_in.reshape(E * N, Lw, d + Z), dh, None, 0.0)
                pred = pred.reshape(E, N, Lw, d)
                _, eh, new_lat = O.encoder_forward(ep, curr.reshape(E * N, Lw, d), eh)
                latent = (1.0 - COEF) * latent + new_lat.reshape(E, N, Z) * COEF
                s[j, :, 0] = ((nxt - pred).abs() * mn).sum((0, 1, 3))
                s[j, :, 1] = torch.clamp(torch.linalg.norm(curr - pred, dim=-1) - THRES, min=0).sum((0, 1))
                lat_j.append(latent.reshape(E * N, Z))
                rec_j.append(pred.reshape(E * N, Lw, d))
            lats.append(torch.stack(lat_j, 1))
            recs.append(torch.stack(rec_j, 1))
            sums.append(s)
        return torch.stack(lats), torch.stack(recs), torch.stack(sums)


def _cmp(got, r64, r32, worst, key, what):
    if float(r64.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, (what, key, "reference is exactly zero")
        return
    e32, err = _grad_err(r32, r64), _grad_err(got, r64)
    print(what, key, "err", err, "e32", e32)
    _worse(worst, key, err)
    _worse(worst, key + "_e32", e32)
    assert err <= _bound(e32), (what, key, err, e32)


def assert_vs_fp64(case, out, worst, what, refs=None):
    (l64, r64, s64), (l32, r32, s32) = refs if refs is not None else (case.reference(torch.float64), case.reference(torch.float32))
    for n in range(case.n_nets):
        if out["latent"] is not None:
            _cmp(out["latent"][n], l64[n], l32[n], worst, "latent", (what, n))
        if out["recon"] is not None:
            _cmp(out["recon"][n], r64[n], r32[n], worst, "recon", (what, n))
        if out["sums"] is not None:
            _cmp(out["sums"][n, ..., 0], s64[n, ..., 0], s32[n, ..., 0], worst, "l1_sums", (what, n))
            _cmp(out["sums"][n, ..., 1], s64[n, ..., 1], s32[n, ..., 1], worst, "stability_sums", (what, n))


# ------------------------------------------------------------------------------------------------ the kernel alone
def check_kernel(device, E, N, Lw, J, d, Z, n_nets):
    """latent, reconstruction and the two sums against fp64, all three in one launch"""
    case = Case(E, N, Lw, J, d, Z, n_nets, device)
    worst = {}
    out = case.run()
    assert out["latent"].shape == (n_nets, E * N, J, Z) and out["recon"].shape == (n_nets, E * N, J, Lw, d)
    assert out["sums"].shape == (n_nets, J, Lw, 2)
    assert_vs_fp64(case, out, worst, (E, N, Lw, J, d, Z, n_nets))
    return worst


def check_output_combinations(device, E=3, N=7, Lw=3, J=4, d=5, Z=8, n_nets=2):
    """every combination of the three optional outputs: what a launch produces does not depend on what else it was asked for
    (bitwise); without the sums no mask is handed over at all; asking for nothing is an error, not a launch"""
    case = Case(E, N, Lw, J, d, Z, n_nets, device, seed=5)
    worst = {}
    refs = case.reference(torch.float64), case.reference(torch.float32)
    full = case.run()
    assert_vs_fp64(case, full, worst, "all three", refs)
    for lat in (False, True):
        for rec in (False, True):
            for sm in (False, True):
                if not (lat or rec or sm):
                    continue
                out = case.run(latent=lat, recon=rec, sums=sm)
                for k, want in (("latent", lat), ("recon", rec), ("sums", sm)):
                    assert (out[k] is not None) == want
                    assert getattr(out["_args"], k) is None or want
                    if want:
                        assert torch.equal(out[k], full[k]), (k, lat, rec, sm)
                if not sm:
                    assert out["_args"].mask is None and out["_args"].part is None
    try:
        case.run(latent=False, recon=False, sums=False)
        raise RuntimeError("a call that asks for nothing was accepted")
    except AssertionError:
        pass
    a = full["_args"]
    keep = (a.latent, a.recon, a.sums)
    a.latent = a.recon = a.sums = None
    try:
        ops._lib(None).call("iplan_beh_eval", a, L.current_stream(device))
        raise AssertionError("a launch that asks for nothing was accepted")
    except L.IplanError:
        pass
    a.latent, a.recon = keep[0], keep[1]
    a.sums, saved_mask = keep[2], a.mask
    a.mask = None
    try:
        ops._lib(None).call("iplan_beh_eval", a, L.current_stream(device))
        raise AssertionError("sums without a mask were accepted")
    except L.IplanError:
        pass
    a.mask = saved_mask
    return worst


def check_sentinel(device, E, N, Lw, J, d, Z, n_nets):
    """the outputs (and the scratch partials) inside buffers pre-filled with a sentinel: every float the launch does not own
    comes back unchanged -- the padding lanes of a ragged last tile write nothing -- and every owned float is written"""
    case = Case(E, N, Lw, J, d, Z, n_nets, device, seed=9)
    ref = case.run()
    a = ref["_args"]
    pad = 64
    rows, tiles = E * N, (E * N + 15) // 16
    sizes = dict(latent=n_nets * rows * J * Z, recon=n_nets * rows * J * Lw * d, sums=n_nets * J * Lw * 2, part=n_nets * J * Lw * 2 * tiles)
    runs = []
    for shift in (0.0, 0.25):
        bufs, sentinels = {}, {}
        for k, n in sizes.items():
            idx = torch.arange(n + 2 * pad, dtype=torch.float32)
            sentinels[k] = 2.5 + shift + (idx % 1021) / 1024.0                # never an output: |latent| <= 1, others differ by the shift
            bufs[k] = sentinels[k].clone().to(device)
            setattr(a, k, bufs[k].data_ptr() + 4 * pad)
        ops._lib(None).call("iplan_beh_eval", a, L.current_stream(device))
        _sync(device)
        for k, n in sizes.items():
            got = bufs[k].cpu()
            assert torch.equal(got[:pad].view(torch.int32), sentinels[k][:pad].view(torch.int32)), (k, "floats in front were written")
            assert torch.equal(got[pad + n:].view(torch.int32), sentinels[k][pad + n:].view(torch.int32)), (k, "floats behind were written")
        runs.append({k: bufs[k][pad:pad + sizes[k]].cpu() for k in sizes})
    for k in ("latent", "recon", "sums"):
        assert torch.equal(runs[0][k].view_as(ref[k]), ref[k].cpu()), k
    for k in sizes:                                                           # written both times: the two sentinels differ everywhere
        assert torch.equal(runs[0][k], runs[1][k]), (k, "an owned float was left unwritten")
    return {}


def check_masks(device, E=3, N=6, Lw=3, J=5, d=5, Z=8, n_nets=2):
    """a window whose target steps are masked out in every env gives exactly 0 L1 sums (whatever the errors are), and so does an
    all-zero mask; the stability sums and the other outputs do not depend on the mask"""
    case = Case(E, N, Lw, J, d, Z, n_nets, device, seed=3)
    worst = {}
    base = case.run()
    j0 = 2
    case.mask[:, :, j0 + 1:j0 + 1 + Lw] = 0.0
    case.upload()
    out = case.run()
    assert_vs_fp64(case, out, worst, "one window masked out")
    assert torch.equal(out["sums"][:, j0, :, 0].cpu(), torch.zeros(n_nets, Lw))
    assert float(out["sums"][:, j0 - 2, :, 0].abs().max()) > 0
    assert torch.equal(out["sums"][..., 1], base["sums"][..., 1]) and torch.equal(out["latent"], base["latent"]) and torch.equal(out["recon"], base["recon"])
    # masked rows are dropped whatever their error is: step T - 2 is nobody's input, only the last target of the last windows --
    # garbage there, under a zero mask, changes no sum
    case.mask[:, 1, case.T - 2] = 0.0
    case.upload()
    ref = case.run(latent=False, recon=False)["sums"]
    case.buf[1, case.T - 1] = 1e30                                           # (buffer step 1 + t holds episode step t)
    case.upload()
    assert torch.equal(case.run(latent=False, recon=False)["sums"], ref)
    case.mask[:] = 0.0
    case.upload()
    out = case.run()
    assert torch.equal(out["sums"][..., 0].cpu(), torch.zeros(n_nets, J, Lw))
    assert torch.equal(out["sums"][..., 1], base["sums"][..., 1])
    return worst


def check_repeatable(device, E=5, N=13, Lw=3, J=4, d=5, Z=8, n_nets=5):
    """three launches, bitwise-equal outputs (an order of summation, not a race, is what this pins)"""
    case = Case(E, N, Lw, J, d, Z, n_nets, device, seed=1)
    first = case.run()
    for _ in range(2):
        again = case.run()
        for k in ("latent", "recon", "sums"):
            assert torch.equal(again[k], first[k]), k
    return {}


def check_invalid_dims(device):
    """J < 1 and d + Z > 16 are refused by the entry point's host check (an IplanError, no launch)"""
    for kw in (dict(E=1, N=3, Lw=3, J=0, d=5, Z=8), dict(E=1, N=3, Lw=3, J=-1, d=5, Z=8), dict(E=1, N=3, Lw=2, J=2, d=12, Z=8)):
        case = Case(n_nets=1, device=device, **kw)
        for want in (dict(latent=True, recon=False, sums=False), dict(latent=True, recon=True, sums=True)):
            try:
                case.run(**want)
                raise AssertionError(("accepted", kw))
            except L.IplanError as e:
                assert "unsupported dims" in str(e), str(e)
    return {}


# ------------------------------------------------------------------------------------------------ against the training path
def check_agrees_with_training(device, E=3, N=6, Lw=3, J=5, d=5, Z=8, n_nets=2):
    """losses formed from iplan_beh_eval's sums and ops.beh_forward(drop_p=0)'s loss, each against the fp64 oracle"""
    case = Case(E, N, Lw, J, d, Z, n_nets, device, seed=2)
    out = case.run(latent=False, recon=False)
    hist_c = case.d_hist
    fwd = ops.beh_forward(case.enc_arena, case.dec_arena, hist_c, case.d_mask, Lw, Z, COEF, THRES, 0.0, seed=0)
    _sync(device)
    wn = ops.beh_window_mask_sums(case.d_mask, Lw).double().cpu()
    s = out["sums"].double().cpu()
    beh = (s[..., 0].sum(2) / (wn * (N * d) + O.EPS) * (d * N)).sum(1) / J
    stab = (s[..., 1].sum(2) / E / Lw).sum(1) / J
    hist = case.view(case.buf)
    worst = {}
    for n in range(n_nets):
        ref = {}
        for dt in (torch.float64, torch.float32):
            ep = {k: v.to(dt) for k, v in case.enc_p[n].items()}
            dp = {k: v.to(dt) for k, v in case.dec_p[n].items()}
            b, st, _ = O.behavior_learn_loss(ep, dp, hist[n].to(dt), case.mask[n], Lw, COEF, None, 0.0, 0.0, THRES)
            ref[dt] = torch.stack([b, st]).double()
        for k, name in ((0, "behavior"), (1, "stability")):
            r64, r32 = ref[torch.float64][k:k + 1], ref[torch.float32][k:k + 1]
            e32 = _grad_err(r32, r64)
            mine = _grad_err(torch.stack([beh, stab], 1)[n, k:k + 1], r64)
            train = _grad_err(fwd["loss"][n, k:k + 1], r64)
            print("net", n, name, "evaluate err", mine, "training forward err", train, "e32", e32)
            _worse(worst, name + "_eval", mine)
            _worse(worst, name + "_train", train)
            _worse(worst, name + "_e32", e32)
            assert mine <= _bound(e32) and train <= _bound(e32), (n, name, mine, train, e32)
    return worst


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_args(device, **kw):
    from iplan_amd.config import default_args
    base = dict(use_cuda=torch.device(device).type == "cuda", max_vehicle_num=5, n_agents=2, episode_limit=9, max_history_len=3,
                behavior_variation_penalty=0.5)
    base.update(kw)
    return default_args("highway", **base)


def _policy(args, seed, cls=None):
    from iplan_amd.nova.stable_behavior_policy import Behavior_policy
    torch.manual_seed(seed)
    return (cls or Behavior_policy)(args, _Log())


def _loaded_policy(args, tmp_path, seed):
    """save -> fresh policy (other weights) -> load; returns (policy, encoder state dicts, decoder state dicts)"""
    src = _policy(args, seed)
    enc = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in src.behavior_encoder]
    dec = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in src.behavior_decoder]
    src.save_models(str(tmp_path))
    pol = _policy(args, seed + 100)
    assert not torch.equal(pol.behavior_decoder[0].state_dict()["decoder.out.weight"].cpu(), dec[0]["decoder.out.weight"])
    pol.load_models([str(tmp_path)])
    return pol, enc, dec


def _rng_states(device):
    st = [torch.get_rng_state(), torch.as_tensor(np.random.get_state()[1].copy())]
    if torch.device(device).type == "cuda":
        st.append(torch.cuda.get_rng_state(device))
    return st


def _batch(args, E, device, seed=6):
    from iplan_amd import synth
    f = synth.make_episode_fields(args, E, seed=seed, terminated_p=0.8)
    f["terminated"][:, args.episode_limit // 2] = 0                          # a zero mid-episode (highway polarity: mask = terminated)
    return f, synth.DictBatch(f, E, args.episode_limit + 1).to(device)


def _policy_reference(args, enc, dec, f, dtype):
    """per agent (beh, stab) from oracle.behavior_learn_loss, and latents / reconstructions / per-step L1 from the restated loop"""
    hist, term = f["history"][:, :-1], f["terminated"][:, :-1]
    E, T, nA, N, d = hist.shape
    Lw, Z = args.max_history_len, args.latent_dim
    J = T - 1 - Lw
    res = dict(beh=[], stab=[], latent=[], recon=[], l1=[], count=[])
    for i in range(nA):
        mask = term[:, :, i, 0]
        ep = {k: v.to(dtype) for k, v in enc[i].items()}
        dp = {k: v.to(dtype) for k, v in dec[i].items()}
        b, s, _ = O.behavior_learn_loss(ep, dp, hist[:, :, i].to(dtype), mask, Lw, args.soft_update_coef, None, 0.0,
                                        args.behavior_variation_penalty, args.thres_small_variation)
        res["beh"].append(b)
        res["stab"].append(s)
        dps = O.strip_prefix(dp, "decoder.")
        latent = torch.zeros(E, N, Z, dtype=dtype)
        eh, dh = torch.zeros(E * N, 32, dtype=dtype), torch.zeros(E * N, 64, dtype=dtype)
        lat_j, rec_j = [], []
        l1, cnt, beh2 = torch.zeros(Lw, dtype=dtype), torch.zeros(Lw, dtype=torch.float64), 0.0
        for j in range(J):
            curr, nxt, mn = O.behavior_windows(hist[:, :, i].to(dtype), mask, j, Lw)
            dec_in = torch.cat([curr, latent[:, :, None, :].expand(E, N, Lw, Z)], dim=-1)
            pred, dh = O.decoder_forward(dps, dec_in.reshape(E * N, Lw, d + Z), dh, None, 0.0)
            pred = pred.reshape(E, N, Lw, d)
            _, eh, new_lat = O.encoder_forward(ep, curr.reshape(E * N, Lw, d), eh)
            latent = (1.0 - args.soft_update_coef) * latent + new_lat.reshape(E, N, Z) * args.soft_update_coef
            l1 += ((nxt - pred).abs() * mn).sum((0, 1, 3))
            cnt += mn[..., 0].double().sum((0, 1))
            beh2 = beh2 + O.masked_l1(nxt, pred, mn, d * N)
            lat_j.append(latent)
            rec_j.append(pred)
        if dtype == torch.float64:                                            # the restatement IS the oracle's loop
            assert abs(float(beh2 / J) - float(b)) <= 1e-12 * max(1.0, abs(float(b)))
        res["latent"].append(torch.stack(lat_j, 1))                           # [E, J, N, Z]
        res["recon"].append(torch.stack(rec_j, 1))                            # [E, J, N, L, d]
        res["l1"].append(l1 / (cnt.to(dtype) * d))
        res["count"].append(cnt)
    out = dict(beh=torch.stack(res["beh"]), stab=torch.stack(res["stab"]), latent=torch.stack(res["latent"], 2),
               recon=torch.stack(res["recon"], 2), l1=torch.stack(res["l1"]), count=torch.stack(res["count"]))
    return out


def check_policy_methods(device, tmp_path, E=3):
    """evaluate / latent_trace on a loaded checkpoint against the oracle: numpy and device inputs, defer=True, every returned
    array; parameters, optimiser state and the generators untouched"""
    args = _e2e_args(device)
    pol, enc, dec = _loaded_policy(args, tmp_path, 11)
    nA, N, Lw, T, d, Z = args.n_agents, args.max_vehicle_num, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    J = T - 1 - Lw
    f, batch = _batch(args, E, device)
    before = dict(enc=pol.enc_arena.data.clone(), dec=pol.dec_arena.data.clone(), rng=_rng_states(device),
                  opt=[str(o.state_dict()) for o in pol.behavior_optimizer])
    res = pol.evaluate(batch, return_latent=True, return_reconstruction=True)
    fin = pol.evaluate(batch, return_latent=True, return_reconstruction=True, defer=True)
    assert callable(fin)
    res2 = fin()
    lean = pol.evaluate(batch)
    assert "latent" not in lean and "reconstruction" not in lean
    hist_np = f["history"][:, :-1].double().numpy()
    tr_np = pol.latent_trace(hist_np)
    tr_dev = pol.latent_trace(f["history"][:, :-1].to(device))
    assert torch.equal(pol.enc_arena.data, before["enc"]) and torch.equal(pol.dec_arena.data, before["dec"])
    assert all(torch.equal(x, y) for x, y in zip(_rng_states(device), before["rng"]))
    assert [str(o.state_dict()) for o in pol.behavior_optimizer] == before["opt"]
    for k in res:
        assert isinstance(res[k], np.ndarray) and np.array_equal(res[k], res2[k], equal_nan=True), k
    for k in lean:
        assert np.array_equal(res[k], lean[k], equal_nan=True), k
    assert res["latent"].shape == (E, J, nA, N, Z) and res["reconstruction"].shape == (E, J, nA, N, Lw, d)
    assert res["behavior_loss"].shape == (nA,) and res["l1_per_step"].shape == (nA, Lw) and res["count"].shape == (nA, Lw)
    assert isinstance(tr_np, np.ndarray) and tr_np.shape == (E, J, nA, N, Z)
    assert torch.is_tensor(tr_dev) and tr_dev.device.type == torch.device(device).type
    assert np.array_equal(tr_dev.cpu().numpy(), tr_np) and np.array_equal(tr_np, res["latent"])
    r64, r32 = _policy_reference(args, enc, dec, f, torch.float64), _policy_reference(args, enc, dec, f, torch.float32)
    worst = {}
    assert np.array_equal(res["count"], r64["count"].numpy()), (res["count"], r64["count"])
    assert (res["count"] > 0).all()
    for key, rk in (("behavior_loss", "beh"), ("stability_loss", "stab"), ("l1_per_step", "l1"), ("latent", "latent"), ("reconstruction", "recon")):
        for i in range(nA):
            sel = (lambda x: x[:, :, i]) if rk in ("latent", "recon") else (lambda x: x[i:i + 1] if x.dim() == 1 else x[i])
            _cmp(sel(torch.as_tensor(res[key])), sel(r64[rk]), sel(r32[rk]), worst, key, ("agent", i))
    assert np.array_equal(res["total_loss"], res["behavior_loss"] + args.behavior_variation_penalty * res["stability_loss"])
    assert (res["stability_loss"] > 0).all()
    return worst


def check_policy_masks(device, E=2):
    """nothing counts at some look-ahead steps / anywhere: finite losses, NaN exactly where count is 0, exact counts"""
    args = _e2e_args(device)
    pol = _policy(args, 17)
    nA, Lw, T = args.n_agents, args.max_history_len, args.episode_limit
    f, _ = _batch(args, E, device)
    from iplan_amd import synth
    f["terminated"][:] = 0
    f["terminated"][:, 1, 0] = 1          # agent 0: only step 1 counts -- the target of window 0 at look-ahead step 0 alone
    f["terminated"][:, 2:, 1] = 1         # agent 1: everything from step 2 on
    res = pol.evaluate(synth.DictBatch(f, E, T + 1).to(device))
    term = f["terminated"][:, :-1, :, 0].double()                                # [E, T, nA]
    J = T - 1 - Lw
    cnt = torch.stack([torch.stack([term[:, 1 + t:1 + t + J, i].sum() for t in range(Lw)]) for i in range(nA)]) * args.max_vehicle_num
    assert np.array_equal(res["count"], cnt.numpy()), (res["count"], cnt)
    assert res["count"][0, 0] > 0 and (res["count"][0, 1:] == 0).all()
    assert np.array_equal(np.isnan(res["l1_per_step"]), res["count"] == 0)
    for k in ("behavior_loss", "stability_loss", "total_loss"):
        assert np.isfinite(res[k]).all(), k
    f["terminated"][:] = 0
    none = pol.evaluate(synth.DictBatch(f, E, T + 1).to(device))
    assert (none["count"] == 0).all() and np.isnan(none["l1_per_step"]).all()
    assert (none["behavior_loss"] == 0).all() and np.isfinite(none["stability_loss"]).all() and np.isfinite(none["total_loss"]).all()
    return {}


def check_dropout_and_rng(device, E=2):
    """a policy built with decoder_dropout = 0.5 returns the same bits as one with 0.0 on the same weights; two calls are
    bitwise equal; no generator moves"""
    results = []
    for p in (0.5, 0.0):
        args = _e2e_args(device, decoder_dropout=p)
        pol = _policy(args, 23)
        f, batch = _batch(args, E, device)
        torch.manual_seed(5)
        rng = _rng_states(device)
        a = pol.evaluate(batch, return_latent=True, return_reconstruction=True)
        b = pol.evaluate(batch, return_latent=True, return_reconstruction=True)
        tr = pol.latent_trace(f["history"][:, :-1].numpy())
        assert all(torch.equal(x, y) for x, y in zip(_rng_states(device), rng))
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(tr, a["latent"])
        results.append(a)
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k], equal_nan=True), k
    return {}


def check_latent_trace_vs_latent_update(device, tmp_path, E=2):
    """latent_trace step j against latent_update driven window by window over the same right-aligned, zero-padded windows, both
    within the bound of the fp64 oracle"""
    args = _e2e_args(device)
    pol, enc, dec = _loaded_policy(args, tmp_path, 29)
    nA, N, Lw, T, d, Z = args.n_agents, args.max_vehicle_num, args.max_history_len, args.episode_limit, args.obs_shape_single, args.latent_dim
    J = T - 1 - Lw
    f, _ = _batch(args, E, device, seed=8)
    hist = f["history"][:, :-1]                                                # [E, T, nA, N, d]
    trace = pol.latent_trace(hist.to(device))
    lat = torch.zeros(E, nA, N, Z, device=device)
    hid = torch.zeros(E, 1, nA, N, args.encoder_rnn_dim, device=device)
    steps = []
    for j in range(J):
        win = torch.zeros(E, nA, N, Lw, d)
        start, plug = max(0, j - Lw + 1), max(0, Lw - j - 1)
        win[:, :, :, plug:] = hist[:, start:j + 1].permute(0, 2, 3, 1, 4)
        lat, hid = pol.latent_update(win.to(device), hid, lat)
        steps.append(lat)
    stepped = torch.stack(steps, 1)                                            # [E, J, nA, N, Z]
    r64, r32 = _policy_reference(args, enc, dec, f, torch.float64), _policy_reference(args, enc, dec, f, torch.float32)
    worst = {}
    for i in range(nA):
        _cmp(trace[:, :, i], r64["latent"][:, :, i], r32["latent"][:, :, i], worst, "trace", ("agent", i))
        _cmp(stepped[:, :, i], r64["latent"][:, :, i], r32["latent"][:, :, i], worst, "stepped", ("agent", i))
        e32 = _grad_err(r32["latent"][:, :, i], r64["latent"][:, :, i])
        assert _grad_err(trace[:, :, i], stepped[:, :, i]) <= 2 * _bound(e32)  # (each within the bound of the same reference)
    return worst


def _keep(args, E, seed):
    gen = torch.Generator().manual_seed(seed)
    J = args.episode_limit - 1 - args.max_history_len
    return (torch.rand(args.n_agents, J, E * args.max_vehicle_num, args.max_history_len, args.decoder_rnn_dim, generator=gen)
            < 1.0 - args.decoder_dropout).to(torch.uint8)


def check_learn_unaffected_by_evaluate(device, E=2):
    """learn() with injected keep flags gives bitwise-equal losses and parameters whether or not evaluate() ran before it"""
    args = _e2e_args(device)
    _, batch = _batch(args, E, device)
    keep = _keep(args, E, 21).to(device)
    results = []
    for with_eval in (False, True):
        pol = _policy(args, 31)
        if with_eval:
            ev = pol.evaluate(batch, return_latent=True)
            assert np.isfinite(ev["total_loss"]).all()
            pol.latent_trace(batch["history"][:, :-1])
        losses = pol.learn(batch, 0, keep=keep)
        pol.join_decoder()
        _sync(device)
        results.append((np.asarray(losses), pol.enc_arena.data.clone(), pol.dec_arena.data.clone()))
    (l0, e0, d0), (l1, e1, d1) = results
    assert np.array_equal(l0, l1) and torch.equal(e0, e1) and torch.equal(d0, d1)
    return {}


def check_evaluate_after_deferred_learn(device, E=2):
    """evaluate() after learn(defer_decoder=True) waits for the decoder update that call left on the side stream.
    (a) It returns the bits of the same deferred learn followed by an explicit join_decoder() and a device synchronisation.
    (b) After the deferred and after the undeferred learn it is within the fp64 bound of the oracle evaluated at that policy's
        OWN post-step parameters -- a call that did not wait would see the previous decoder, one Adam step (lr 1e-4 per entry)
        away.  The two learn forms contract the decoder's weight gradients in different shapes and agree to rounding, not to
        the bit (tests/oracle_checks.py: check_deferred_equals_inline holds them to 1e-6), so the two evaluations are compared
        through their references; where the update runs in line (no GPU: the same code either way) they are bitwise equal."""
    args = _e2e_args(device)
    f, batch = _batch(args, E, device)
    keep = _keep(args, E, 22).to(device)
    nA = args.n_agents
    results, worst = {}, {}
    for form in ("inline", "deferred", "deferred_joined"):
        pol = _policy(args, 37)
        before = pol.evaluate(batch)
        pol.learn(batch, 0, keep=keep, defer_decoder=form != "inline")
        if form == "deferred_joined":
            pol.join_decoder()
            _sync(device)
        after = pol.evaluate(batch, return_latent=True, return_reconstruction=True)
        assert not np.array_equal(after["behavior_loss"], before["behavior_loss"])          # the step moved the parameters
        results[form] = after
        pol.join_decoder()
        _sync(device)
        enc = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in pol.behavior_encoder]
        dec = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in pol.behavior_decoder]
        r64, r32 = _policy_reference(args, enc, dec, f, torch.float64), _policy_reference(args, enc, dec, f, torch.float32)
        for key, rk in (("behavior_loss", "beh"), ("stability_loss", "stab"), ("reconstruction", "recon"), ("latent", "latent")):
            for i in range(nA):
                sel = (lambda x: x[:, :, i]) if rk in ("latent", "recon") else (lambda x: x[i:i + 1])
                _cmp(sel(torch.as_tensor(after[key])), sel(r64[rk]), sel(r32[rk]), worst, key, (form, "agent", i))
    for k in results["deferred"]:
        assert np.array_equal(results["deferred"][k], results["deferred_joined"][k], equal_nan=True), k
        if torch.device(device).type != "cuda":
            assert np.array_equal(results["deferred"][k], results["inline"][k], equal_nan=True), k
    return worst


def check_subclasses_refuse(device):
    """the hard-update and fully-connected policies have other window geometry / networks: both methods raise"""
    from iplan_amd.nova import behavior_FC_policy, behavior_policy
    for mod, kw in ((behavior_policy, {}), (behavior_FC_policy, dict(behavior_fully_connected=True))):
        args = _e2e_args(device, **kw)
        pol = _policy(args, 41, cls=mod.Behavior_policy)
        _, batch = _batch(args, 1, device)
        for call in (lambda: pol.evaluate(batch), lambda: pol.latent_trace(batch["history"][:, :-1])):
            try:
                call()
                raise AssertionError("accepted")
            except NotImplementedError:
                pass
    return {}


# ------------------------------------------------------------------------------------------------ GPU only: device memory
def check_device_memory(device, E=8, N=17, T=30, Lw=10, n_nets=5):
    """peak extra device memory of evaluate() with no optional outputs, against the activation records the training forward
    allocates at the same shape: below one sixteenth (the records are 688 floats per chain-step, the per-tile partials 2 floats
    per 16 chains per (j, t))"""
    assert torch.device(device).type == "cuda"
    args = _e2e_args(device, max_vehicle_num=N, n_agents=n_nets, episode_limit=T, max_history_len=Lw)
    pol = _policy(args, 43)
    _, batch = _batch(args, E, device)
    v = pol._episode_views(batch)
    fwd = ops.beh_forward(pol.enc_arena, pol.dec_arena, v["hist"], v["mask"], Lw, args.latent_dim, args.soft_update_coef,
                          args.thres_small_variation, 0.0, seed=0)
    torch.cuda.synchronize()
    records = sum(fwd[k].numel() * fwd[k].element_size() for k in ("saved_dec", "saved_enc"))
    del fwd
    pol.evaluate(batch)                                                        # (warm: the library and the copy stream exist)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(device)
    level = torch.cuda.memory_allocated(device)
    res = pol.evaluate(batch)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(device) - level
    print("evaluate peak extra bytes", extra, "training records bytes", records)
    assert np.isfinite(res["total_loss"]).all()
    assert 0 <= extra < records / 16, (extra, records)
    return dict(extra_bytes=float(extra), record_bytes=float(records))
