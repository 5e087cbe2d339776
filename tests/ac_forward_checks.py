"""TEST INFRASTRUCTURE: the actor / critic forward kernel alone (csrc/actor_critic.hip, csrc/ac_fwd_body.h through ops.ac_forward) in each
of its launch forms, on whatever library is active -- the host emulator in tests/test_emu_ac_forward.py, the gfx950 build in
tests/test_gpu_ac_forward.py.

Ground truth: oracle.actor_logits / actor_evaluate / critic_value on every row by itself (each row has its own recorded GRU state), in
fp64 and in fp32, on the features of oracle.build_inputs_train plus the one-hots as policy_trace_checks.walk_reference assembles them.
Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor and net, bound = max(1e-5, E32_FACTOR x the fp32
oracle's own error against fp64 on the same tensor).  The only other numbers are the two margins inside which an argmax may
legitimately differ from the fp64 one: 10 x 1e-5 of the larger probability (greedy), 1e-4 between the two largest keys (sampled).

Rows are laid out E x S with T = S and T_phys = S + 1 inside larger buffers (policy_trace_checks.Case), so the physical-row mapping
pr = (r / T) T_phys + r % T is always exercised.  Every case holds one row with exactly one available action and one row -- the last,
i.e. a valid row of the ragged tile -- with none.  The checks never touch ``L.use_library_for_tests``; each returns what it measured."""
import functools

import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests import policy_trace_checks as PC
from tests.oracle_checks import _grad_err
from tests.policy_trace_checks import M, TOL, _bits, _bound, _sync, _worse, assert_same_bits, lowest_argmax

FORMS = ("stream", "stream_packed", "stats", "pre", "pre16", "rollout", "rollout_kw2", "rollout_kw4", "rollout_kw8", "module", "ks8_stats")
KW_OF = {"rollout": "1", "rollout_kw2": "2", "rollout_kw4": "4", "rollout_kw8": "8"}
TWO_PASS = ("stream", "stats", "ks8_stats")
FOLDED = ("rollout", "rollout_kw4", "module")
THREE = ("stream", "rollout_kw4", "module")
# rows -> (E, S)
ROWS = {1: (1, 1), 16: (8, 2), 17: (17, 1), 32: (16, 2), 33: (11, 3), 256: (64, 4), 257: (257, 1)}
ROWS_ALL = (1, 16, 17, 33)
ROWS_STREAM = (32, 256, 257)           # edges of a wave's two row tiles and of a workgroup's 16 (streaming form only)
FLOAT_OUTS = ("logp", "entropy", "probs", "values", "h_actor", "h_critic")


def dims_of(rows, nA=2, N=3, d=5, n_act=5):
    E, S = ROWS[rows]
    return (nA, E, S, N, d, n_act)


# K-axis cases, 17 rows each: (id, dims, options)
K_CASES = [
    ("smallest_F", dims_of(17, N=2), {}),                                   # empty K shares at kw8
    ("kmap_edge", dims_of(17), dict(latent=6)),                             # N w ends in padded k-tiles
    ("no_gat", dims_of(17), dict(gat=False)),
    ("no_beh", dims_of(17), dict(beh=False)),
    ("no_onehots", dims_of(17), dict(last_action=False, agent_id=False, last64=True)),
    ("tanh", dims_of(17), dict(tanh=True)),
    ("head16", dims_of(17, n_act=16), {}),
    ("head1", dims_of(17, n_act=1), {}),
    ("product_layout", dims_of(17, nA=5, N=5, d=7), {}),
]
K_FORMS = ("stream", "rollout_kw4", "rollout_kw8", "module")
SWEEP_SHIFTS = (0.0, 1.0, 4.0)
# seeds of the Exp(1) draws of check 4, chosen on the CPU from the fp64 reference's margins alone (pick_q_seed): no row of the case
# lies inside the 1e-4 margin
Q_SEEDS = {33: 0, 17: 0}


class AcCase(PC.Case):
    """policy_trace_checks.Case with a recorded GRU state for EVERY row, an optional constant added to every feature of the three
    sources, and a row without any available action"""

    def __init__(self, dims, device, seed=0, poison=False, last64=False, shift=0.0, tie=None, **opt):
        super().__init__(dims, device, seed=seed, poison=poison, last64=last64, **opt)
        nA, E, S, N, d, n_act = dims
        gen = torch.Generator().manual_seed(900 + seed + sum(dims))
        for key in ("ha", "hc"):
            self.buf[key][:, :S, :, 4:4 + M] = torch.randn(E, S, nA, M, generator=gen) * 0.3
        if shift:
            for key, w in (("history", d), ("att", self.args.attention_dim), ("beh", self.args.latent_dim)):
                self.buf[key][:, :S, :, self.PAD:self.PAD + N * w] += shift
        with torch.no_grad():          # values around +4 instead of around 0 (policy_trace_checks.check_replays_rollout: a value's rounding
            for c in self.mac.critics:  # error is set by the 64 products its head sums; the rule divides by the largest |value| of a net's
                c.v_out.bias.add_(4.0)  # rows, which at rows = 1 is ONE value that may sit near zero).  Bounds and cases are unchanged.
        self.buf["actions"][..., 0] = 99                                         # junk around the recorded actions in every case
        self.buf["actions"][:, S] = 99
        self.one_row, self.none_row = (0, 0, 0), (E - 1, S - 1, nA - 1)         # (environment, step, net)
        self.buf["avail"][E - 1, S - 1, nA - 1, 1:1 + n_act] = 0
        if tie is not None:            # two head rows made equal, only those two actions available: every row is an exact tie
            lo, hi = tie
            with torch.no_grad():
                for m in self.mac.agents:
                    p = dict(m.named_parameters())
                    p["act.action_out.linear.weight"][hi].copy_(p["act.action_out.linear.weight"][lo])
                    p["act.action_out.linear.bias"][hi].copy_(p["act.action_out.linear.bias"][lo])
            self.buf["avail"][:, :S, :, 1:1 + n_act] = 0
            self.buf["avail"][:, :S, :, 1 + lo] = 1
            self.buf["avail"][:, :S, :, 1 + hi] = 1
        self.upload()

    @property
    def rows(self):
        return len(self.order) * self.dims[2]

    def spec(self, all_rows=False):
        nA, _, S, N, d, n_act = self.dims
        a, D = self.args, self.dbuf
        sl = slice(None) if all_rows else slice(0, S)
        srcs = []
        for key, w in self.widths:
            v = D[key][:, sl, :, self.PAD:self.PAD + N * w]
            assert v.untyped_storage().nbytes() > 4 * v.numel()                    # a view into a larger buffer, not a packed copy
            srcs.append((v, w, v.stride(2), v.stride(1)))
        last = D["last"][:, sl, :, 0]
        spec = ops.AcFeatureSpec(N, srcs, n_actions=n_act if a.obs_last_action else 0, last_action=last if a.obs_last_action else None,
                                 la_strides=(last.stride(2), last.stride(1)), n_id=nA if a.obs_agent_id else 0,
                                 T=S + 1 if all_rows else S, T_phys=S + 1)
        assert spec.F == self.mac.input_shape
        return spec

    def ln_stats(self):
        """the critics-only ln_stats_mode = 1 launch over all physical rows that IPPOLearner runs first"""
        nA, _, S = self.dims[:3]
        E = len(self.order)
        hc = self.dbuf["hc"][:, :, :, 4:4 + M]
        ln = torch.full((nA, E * (S + 1), 2), float("nan"), device=self.device)
        ops.ac_forward(None, self.mac.critic_arena, 1, self.spec(True), E * (S + 1), nA, h_critic=hc, h_strides=(hc.stride(2), hc.stride(1)),
                       ksplit=1, want_h=False, ln_stats=ln, ln_stats_mode=1)
        return ln

    def run(self, form, mp, mode=2, which=2, save=False, q=None, actions=None, dest=None):
        """ops.ac_forward in launch form ``form`` over all rows; ``mp``: the test's monkeypatch (environment knobs).  ``actions``: an
        int64 buffer shaped like the case's own; ``dest``: in-place destinations (h_out / actions_out / onehot_out)"""
        nA, _, S, N, d, n_act = self.dims
        rows, D, mac = self.rows, self.dbuf, self.mac
        mp.setenv("IPLAN_AC_KSPLIT_WG", KW_OF.get(form, "1"))
        if form == "pre16":
            mp.setenv("IPLAN_AC_PRE_WAVES", "16")
        else:
            mp.delenv("IPLAN_AC_PRE_WAVES", raising=False)
        spec = self.spec()
        ha, hc = D["ha"][:, :, :, 4:4 + M], D["hc"][:, :, :, 4:4 + M]             # [E, S + 1, nA, M]: physical rows e (S + 1) + s
        av = D["avail"][:, :, :, 1:1 + n_act]
        ac = (D["actions"] if actions is None else actions)[:, :, :, 1]
        kw = dict(h_actor=ha, h_critic=hc, h_strides=(ha.stride(2), ha.stride(1)), avail=av, avail_strides=(av.stride(2), av.stride(1)),
                  mode=mode, n_actions=n_act, want_probs=True, want_entropy=True, save=save)
        if mode == 2:
            kw.update(actions_in=ac, act_strides=(ac.stride(2), ac.stride(1)))
        if mode == 1:
            kw["q_noise"] = q
        kw.update(dest or {})
        if form == "stream":
            kw.update(ksplit=1)
        elif form == "stream_packed":
            kw.update(ksplit=1, packed=mac.fc1_pack.get(spec))
        elif form == "stats":
            kw.update(ksplit=1, ln_stats=self.ln_stats(), ln_stats_mode=2)
        elif form in ("pre", "pre16"):
            assert which == 2
            ln = self.ln_stats()
            kw.update(ksplit=1, ln_stats=ln, ln_stats_mode=2, xhat=ops.ac_xhat_pack(spec, rows, nA, ln))
        elif form in KW_OF:
            kw.update(ksplit=8, packed=mac.fc1_pack.get(spec, fold=True))
        elif form == "module":
            kw.update(ksplit=8)
        elif form == "ks8_stats":
            kw.update(ksplit=8, ln_stats=self.ln_stats(), ln_stats_mode=2)
        else:
            raise ValueError(form)
        out = ops.ac_forward(mac.actor_arena, mac.critic_arena, which, spec, rows, nA, **kw)
        _sync(self.device)
        a = out["_args"]
        assert a.ksplit_wg == (int(KW_OF[form]) if form in KW_OF and form != "rollout" else 0), (form, a.ksplit_wg)
        assert bool(a.fc1_pre) == (form in ("pre", "pre16")) and bool(a.saved) == bool(save)
        if a.ksplit_wg:                # the tickets: every unit's counter is back at zero
            assert int(out["_keep"][13][1].abs().sum()) == 0, (form, "a ticket counter was left non-zero")
        return out

    def features(self, i, dtype):
        """[E, S, F] of net i in ``dtype``: oracle.build_inputs_train plus the one-hots as walk_reference assembles them"""
        nA, E, S, N, d, n_act = self.dims
        gat, beh, last_action, agent_id = self.flags
        f = self.fields(i)
        x = O.build_inputs_train(i, f["history"].to(dtype), f["att"].to(dtype), f["beh"].to(dtype), torch.zeros(E, S, n_act, dtype=dtype), nA, gat, beh)
        parts = [x[..., :x.shape[-1] - n_act - nA]]
        if last_action:
            oh = torch.zeros(E, S, n_act, dtype=dtype)
            oh.scatter_(-1, f["last"].clamp_min(0).unsqueeze(-1), (f["last"] >= 0).to(dtype).unsqueeze(-1))
            parts.append(oh)
        if agent_id:
            idoh = torch.zeros(E, S, nA, dtype=dtype)
            idoh[..., i] = 1
            parts.append(idoh)
        return torch.cat(parts, -1)

    def reference(self, dtype):
        """dict of [nA, rows, ...] tensors in ``dtype`` (computed once, never modified)"""
        return _reference(self, dtype)

    def avail_rows(self):
        nA, E, S, _, _, n_act = self.dims
        return self.buf["avail"][:, :S, :, 1:1 + n_act].permute(2, 0, 1, 3).reshape(nA, E * S, n_act)

    def row_index(self, where):
        e, s, i = where
        return i, e * self.dims[2] + s


@functools.lru_cache(maxsize=None)
def _reference(case, dtype):
    nA, E, S, N, d, n_act = case.dims
    rows = E * S
    ap, cp = PC._params(case.mac, dtype)
    relu = case.args.use_ReLU
    out = {k: [] for k in FLOAT_OUTS}
    for i in range(nA):
        f = case.fields(i)
        x = case.features(i, dtype).reshape(rows, -1)
        ha = case.buf["ha"][:, :S, i, 4:4 + M].reshape(rows, M).to(dtype)
        hc = case.buf["hc"][:, :S, i, 4:4 + M].reshape(rows, M).to(dtype)
        av = f["avail"].reshape(rows, n_act)
        logits, ha_n = O.actor_logits(ap[i], x, ha, av, use_relu=relu)
        la = torch.log_softmax(logits, -1)
        lp, _ = O.actor_evaluate(ap[i], x, ha, f["actions"].reshape(rows), av, use_relu=relu)
        v, hc_n = O.critic_value(cp[i], x, hc, use_relu=relu)
        pr = la.exp()
        for k, t in (("probs", pr), ("entropy", -(pr * la.clamp_min(torch.finfo(dtype).min)).sum(-1)), ("logp", lp[:, 0]), ("values", v[:, 0]),
                     ("h_actor", ha_n), ("h_critic", hc_n)):
            out[k].append(t)
    return {k: torch.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def get_case(dims, device, opt=(), seed=0, poison=False, shift=0.0, tie=None):
    return AcCase(dims, device, seed=seed, poison=poison, shift=shift, tie=tie, **dict(opt))


def _opt(opt):
    return tuple(sorted(dict(opt).items()))


def errors_vs_fp64(case, got, keys=FLOAT_OUTS):
    """{key: (worst error over the nets, the fp32 oracle's error at that net)}"""
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    res = {}
    for k in keys:
        if k not in got:
            continue
        g = got[k].cpu()
        for i in range(g.shape[0]):
            err, e32 = _grad_err(g[i], r64[k][i]), _grad_err(r32[k][i], r64[k][i])
            if k not in res or err / _bound(e32) > res[k][0] / _bound(res[k][1]):
                res[k] = (err, e32)
    return res


def assert_vs_fp64(case, got, worst, what, keys=FLOAT_OUTS):
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    for k in keys:
        if k not in got:
            continue
        g = got[k].cpu()
        assert g.shape == r64[k].shape, (what, k, g.shape)
        for i in range(g.shape[0]):
            err, e32 = _grad_err(g[i], r64[k][i]), _grad_err(r32[k][i], r64[k][i])
            print(what, k, "net", i, "err", err, "e32", e32)
            _worse(worst, k, err)
            _worse(worst, k + "_e32", e32)
            assert err <= _bound(e32), (what, k, i, err, e32)
    if "probs" in got:
        p = got["probs"].cpu().double()
        for i in range(p.shape[0]):
            e32 = _grad_err(r32["probs"][i], r64["probs"][i])
            off = (p[i].sum(-1) - 1).abs().max().item()
            _worse(worst, "probs_sum", off)
            assert off <= _bound(e32), (what, "probs do not sum to 1", i, off)


def assert_head_edges(case, got, what, mode2=True):
    """exact zeros at unavailable actions; the one-available row; the no-available row against the oracle's uniform distribution"""
    n_act = case.dims[5]
    avail = case.avail_rows()
    probs = got["probs"].cpu()
    some = avail.sum(-1) > 0
    masked = (avail == 0) & some.unsqueeze(-1)
    assert torch.equal(probs[masked], torch.zeros_like(probs[masked])), (what, "an unavailable action has a non-zero probability")
    i, r = case.row_index(case.one_row)
    assert int(avail[i, r].sum()) == 1
    assert torch.equal(probs[i, r], avail[i, r].float()), (what, "one available action: probs are not one-hot", probs[i, r])
    assert got["entropy"][i, r].item() == 0.0, (what, "one available action: entropy", got["entropy"][i, r].item())
    if mode2:
        assert got["logp"][i, r].item() == 0.0, (what, "one available action: logp", got["logp"][i, r].item())
    i, r = case.row_index(case.none_row)
    assert int(avail[i, r].sum()) == 0
    r64 = case.reference(torch.float64)
    for k in ("probs", "entropy") + (("logp",) if mode2 else ()):
        ref = r64[k][i, r]
        diff = (got[k][i, r].cpu().double() - ref).abs().max().item()
        assert diff <= TOL * max(ref.abs().max().item(), 1e-30), (what, "no available action", k, got[k][i, r].tolist(), ref.tolist())


# ------------------------------------------------------------------------------------------------ 1, 2: against fp64, mode 2
def check_vs_fp64(device, mp, form, dims, opt=(), which=2, save=False, shift=0.0):
    """every output of every net against fp64 under the rule; mode 2's logp of the recorded action (read through strides from an
    int64 buffer with junk around it); probs sum to 1; the head edges"""
    case = get_case(dims, device, _opt(opt), shift=shift)
    what = (form, dims, dict(opt), which, save)
    got = case.run(form, mp, which=which, save=save)
    want = {0: {"logp", "entropy", "probs", "h_actor"}, 1: {"values", "h_critic"}}
    want[2] = want[0] | want[1]
    assert {k for k in got if k in FLOAT_OUTS} == want[which], (what, sorted(got))
    for k in FLOAT_OUTS:
        if k in got:
            assert torch.isfinite(got[k]).all(), (what, k, "not finite")
    worst = {}
    assert_vs_fp64(case, got, worst, what)
    if which != 1:
        assert_head_edges(case, got, what)
    return worst


# ------------------------------------------------------------------------------------------------ 3: head, mode 0
def _top_two(keys):
    if keys.shape[-1] == 1:
        return keys[..., 0], torch.full_like(keys[..., 0], -float("inf"))
    top = keys.topk(2, -1).values
    return top[..., 0], top[..., 1]


def check_greedy(device, mp, form, rows=33):
    """actions_out == the lowest-index argmax of the kernel's own probs, exactly, and == the fp64 argmax wherever the two largest fp64
    probabilities differ by more than 10 x 1e-5 of the larger"""
    case = get_case(dims_of(rows), device)
    got = case.run(form, mp, mode=0)
    acts = got["actions"].cpu()
    assert acts.dtype == torch.int64
    assert torch.equal(acts, lowest_argmax(got["probs"].cpu())), (form, "actions are not the lowest-index argmax of the returned probs")
    p64 = case.reference(torch.float64)["probs"]
    a, b = _top_two(p64)
    clear = (a - b) > 10 * TOL * a
    assert torch.equal(acts[clear], p64.argmax(-1)[clear]), (form, "greedy action differs from the fp64 argmax outside the margin")
    assert_head_edges(case, got, (form, "mode 0"), mode2=False)
    return {"rows_inside_margin": float((~clear).sum())}, acts, clear


# ------------------------------------------------------------------------------------------------ 4: head, mode 1
def _q_noise(case, seed):
    nA, E, S, _, _, n_act = case.dims
    gen = torch.Generator().manual_seed(seed)
    return -torch.log(torch.rand(nA, E * S, n_act, generator=gen).clamp_min(1e-20))           # Exp(1)


def _sample_margin(case, q):
    keys = case.reference(torch.float64)["probs"] / q.double()
    a, b = _top_two(keys)
    return keys, (a - b) > 1e-4 * a


def pick_q_seed(rows, tries=50):
    """the first seed whose Exp(1) draw leaves no row of the case inside the margin, from the fp64 reference alone (CPU)"""
    case = get_case(dims_of(rows), "cpu")
    for seed in range(tries):
        if bool(_sample_margin(case, _q_noise(case, seed))[1].all()):
            return seed
    raise AssertionError("no seed found")


def check_sampled(device, mp, form, rows=33):
    """actions_out == the fp64 argmax(p64 / q) on every row whose two largest fp64 keys differ, relatively, by more than 1e-4 (no row is
    inside that margin at the committed seed); logp == the kernel's own mode-2 log-prob of the chosen action, in bits"""
    case = get_case(dims_of(rows), device)
    nA, E, S, _, _, n_act = case.dims
    q = _q_noise(case, Q_SEEDS[rows])
    keys, clear = _sample_margin(case, q)
    skipped = int((~clear).sum())
    assert skipped == 0, ("rows inside the margin at the committed seed", skipped)
    got = case.run(form, mp, mode=1, q=q.to(device).contiguous())
    acts = got["actions"].cpu()
    assert torch.equal(acts[clear], keys.argmax(-1)[clear]), (form, "sampled action differs from the fp64 argmax of p / q")
    assert (case.avail_rows().gather(-1, acts.unsqueeze(-1))[..., 0] == 1)[case.avail_rows().sum(-1) > 0].all(), (form, "an unavailable action was drawn")
    abuf = torch.full((E, S + 1, nA, 2), 99, dtype=torch.int64)
    abuf[:, :S, :, 1] = acts.reshape(nA, E, S).permute(1, 2, 0)
    again = case.run(form, mp, mode=2, actions=abuf.to(device))
    assert_same_bits(got, again, (form, "mode 1 against mode 2 on the chosen actions"), ("logp", "entropy", "probs", "values", "h_actor", "h_critic"))
    return {"skipped": float(skipped)}, acts, clear


def check_ties(device, mp, form, rows=17, pair=(1, 3)):
    """two available actions with equal logits (one head row copied onto the other): the lower index wins in mode 0, and in mode 1 under
    equal q"""
    case = get_case(dims_of(rows), device, seed=3, tie=pair)
    nA, E, S, _, _, n_act = case.dims
    g0 = case.run(form, mp, mode=0)
    p = g0["probs"].cpu()
    assert torch.equal(_bits(p[..., pair[0]]), _bits(p[..., pair[1]])), (form, "the two tied probabilities differ in bits")
    assert (p[..., pair[0]] > 0.4).all()
    assert (g0["actions"].cpu() == pair[0]).all(), (form, "mode 0: a tie did not go to the lower index")
    q = _q_noise(case, 5)
    q[..., pair[1]] = q[..., pair[0]]
    g1 = case.run(form, mp, mode=1, q=q.to(device).contiguous())
    assert (g1["actions"].cpu() == pair[0]).all(), (form, "mode 1: a tie did not go to the lower index")
    return {}


# ------------------------------------------------------------------------------------------------ 5: write-back
def _carve(rows, nA, width, device, dtype=torch.float32):
    """a [rows, nA, width] view (rows 2 .., columns 3 ..) of a sentinel-filled [rows + 18, nA, width + 5] buffer: the 16 rows behind
    the view are where a store without its row guard would land"""
    shape = (rows + 18, nA, width + 5)
    n = shape[0] * shape[1] * shape[2]
    if dtype == torch.int64:
        sent = (torch.arange(n, dtype=torch.int64) * 7 + 1000).view(shape)
    else:
        sent = (2.5 + (torch.arange(n, dtype=torch.float32) % 1021) / 1024.0).view(shape)
    buf = sent.clone().to(device)
    view = buf[2:2 + rows, :, 3:3 + width]
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[2:2 + rows, :, 3:3 + width] = True
    return sent, buf, view, mask


def check_write_back(device, mp, form, rows, mode):
    """h_out / actions_out / onehot_out as strided views into sentinel-filled buffers, the way select_actions_ippo(write_back=True) passes
    them: the contiguous launch's bits, onehot == one_hot(actions), no sentinel outside the views changed (ragged last tile included)"""
    case = get_case(dims_of(rows), device)
    nA, n_act = case.dims[0], case.dims[5]
    q = _q_noise(case, Q_SEEDS.get(rows, 0)).to(device).contiguous() if mode == 1 else None
    base = case.run(form, mp, mode=mode, q=q)
    hA, hC, ac, oh = (_carve(rows, nA, M, device), _carve(rows, nA, M, device), _carve(rows, nA, 1, device, torch.int64),
                      _carve(rows, nA, n_act, device))
    strides = lambda v: (v.stride(1), v.stride(0))  # noqa: E731
    av = ac[2][:, :, 0]
    dest = dict(h_out=(hA[2], hC[2], strides(hA[2])), actions_out=(av, strides(av)), onehot_out=(oh[2], strides(oh[2])))
    got = case.run(form, mp, mode=mode, q=q, dest=dest)
    assert "h_actor" not in got and "actions" not in got
    assert_same_bits(got, base, (form, rows, "write-back launch"), ("logp", "entropy", "probs", "values"))
    for name, (sent, buf, view, mask), ref in (("h_actor", hA, base["h_actor"]), ("h_critic", hC, base["h_critic"]),
                                               ("actions", ac, base["actions"].unsqueeze(-1))):
        assert torch.equal(_bits(view.permute(1, 0, 2)), _bits(ref)), (form, rows, name, "differs from the contiguous output")
        host = buf.cpu()
        assert torch.equal(host[~mask], sent[~mask]), (form, rows, name, "an element outside the view was written")
    acts = base["actions"].cpu()
    assert torch.equal(oh[2].cpu().permute(1, 0, 2), torch.nn.functional.one_hot(acts, n_act).float()), (form, rows, "onehot_out is not one_hot(actions_out)")
    assert torch.equal(oh[1].cpu()[~oh[3]], oh[0][~oh[3]]), (form, rows, "onehot_out: an element outside the view was written")
    return {}


# ------------------------------------------------------------------------------------------------ 6: reads only what it owns
def check_poison(device, mp, form, rows=33):
    """NaN in every float the views do not own, junk in every integer: every output finite and the bits of the clean run"""
    clean, dirty = get_case(dims_of(rows), device), get_case(dims_of(rows), device, poison=True)
    for k in ("history", "att", "beh", "ha", "hc"):
        assert torch.isnan(dirty.buf[k]).any() and not torch.isnan(clean.buf[k]).any()
    a, b = clean.run(form, mp), dirty.run(form, mp)
    for k in FLOAT_OUTS:
        assert torch.isfinite(b[k]).all(), (form, k, "not finite")
    assert_same_bits(a, b, (form, "read something outside its views"), FLOAT_OUTS)
    q = _q_noise(clean, Q_SEEDS[rows]).to(device).contiguous()
    a, b = clean.run(form, mp, mode=1, q=q), dirty.run(form, mp, mode=1, q=q)
    assert_same_bits(a, b, (form, "mode 1: read something outside its views"), FLOAT_OUTS + ("actions",))
    return {}


# ------------------------------------------------------------------------------------------------ 7: row independence
def check_row_independence(device, mp, form, rows=33):
    """the environments reversed, and a subset of them: rows move to other lanes, tiles and workgroups, their output bits stay (no form
    sums across rows)"""
    case = get_case(dims_of(rows), device)
    nA, E, S = case.dims[:3]
    full = case.run(form, mp)
    per_env = lambda t, n: t.reshape(nA, n, S, *t.shape[2:])  # noqa: E731
    try:
        for order in (list(range(E - 1, -1, -1)), [E - 1, 3, 7, 0, 5]):
            case.upload(order)
            part = case.run(form, mp)
            for k in FLOAT_OUTS:
                assert torch.equal(_bits(per_env(part[k], len(order))), _bits(per_env(full[k], E)[:, order])), (form, k, order, "a row's bits moved")
    finally:
        case.upload()
    return {}


# ------------------------------------------------------------------------------------------------ 8: repeatability and the tickets
def check_repeatable(device, mp, form, rows=33, reps=3):
    """``reps`` launches in a row: identical bits; Case.run asserts after each that every ticket counter reads zero"""
    case = get_case(dims_of(rows), device)
    first = case.run(form, mp, mode=0)
    assert first["_args"].ksplit_wg == int(KW_OF[form])
    for _ in range(reps - 1):
        assert_same_bits(case.run(form, mp, mode=0), first, (form, "repeat"), FLOAT_OUTS + ("actions",))
    return {}


def check_kw_actions_agree(device, mp, rows=33):
    """kw 1 / 2 / 4 / 8: the same greedy and sampled actions wherever the margins of checks 3 and 4 hold"""
    res = {}
    for form in KW_OF:
        _, g, g_clear = check_greedy(device, mp, form, rows)
        _, s, s_clear = check_sampled(device, mp, form, rows)
        res[form] = (g, s)
    g1, s1 = res["rollout"]
    for form, (g, s) in res.items():
        assert torch.equal(g[g_clear], g1[g_clear]) and torch.equal(s[s_clear], s1[s_clear]), (form, "actions differ from kw = 1")
    return {}


# ------------------------------------------------------------------------------------------------ 9: refusals
def check_refusals(device, mp):
    """every condition of ac_fwd_check: non-zero, a message, nothing launched (sentinel-filled outputs stay as they were)"""
    case = get_case(dims_of(33), device)
    lib = ops._lib(None)
    EINVAL = PC._codes()
    stream = L.C.c_void_p(L.current_stream(torch.device(device)) or 0)
    good = case.run("stream", mp)
    nA, rows, n_act = case.dims[0], case.rows, case.dims[5]
    q = _q_noise(case, 0).to(device).contiguous()
    scratch = torch.zeros(2 * nA * rows * L.AC_SAVE_FLOATS, device=device)
    count = 0

    def refused(out, fields):
        nonlocal count
        a = out["_args"]
        for k in FLOAT_OUTS:
            if k in out:
                out[k].fill_(7.5)
        _sync(device)
        keep = {}
        for k, v in fields.items():
            obj, name = (a, k) if "." not in k else (getattr(a, k.split(".")[0]), k.split(".")[1])
            keep[k] = (obj, name, getattr(obj, name))
            setattr(obj, name, v)
        rc = lib.c.iplan_ac_fwd(L.C.byref(a), stream)
        msg = lib.c.iplan_last_error().decode()
        for obj, name, v in keep.values():
            setattr(obj, name, v)
        _sync(device)
        assert rc == EINVAL and "iplan_ac_fwd" in msg, (fields, rc, msg)
        for k in FLOAT_OUTS:
            if k in out:
                assert bool((out[k] == 7.5).all()), (fields, k, "a refused call wrote an output")
        count += 1

    out = case.run("stream", mp)
    assert case.dims[2] >= 2
    for fields in (dict(ksplit=2), dict(which=3), dict(rows=0), {"feat.T_phys": case.dims[2] - 1}, {"actor.n_out": 0}, {"actor.n_out": 17},
                   dict(mode=1, q_noise=None), dict(actions_in=None)):
        refused(out, fields)
    out = case.run("pre", mp)
    for fields in (dict(ksplit=8), dict(ln_stats=None), dict(ln_stats_mode=0)):
        refused(out, fields)
    out = case.run("rollout_kw4", mp, mode=1, q=q)
    for fields in (dict(ksplit_wg=9), dict(saved=scratch.data_ptr()), dict(packed_actor=None), dict(packed_critic=None), dict(ln_stats_mode=1),
                   dict(ks_count=None), dict(ksplit=1)):
        refused(out, fields)
    assert int(out["_keep"][13][1].abs().sum()) == 0
    assert_same_bits(case.run("stream", mp), good, "after the refusals", FLOAT_OUTS)
    return {"refused": float(count)}


# ------------------------------------------------------------------------------------------------ 10: LayerNorm(F) conditioning sweep
def _one_pass_fp32(x):
    """the fp32 restatement of the folded form's statistics, mean(x^2) - mean(x)^2 -> relative error of rstd against fp64, worst row"""
    x32, x64 = x.float(), x.double()
    mu = x32.mean(-1)
    rstd32 = 1.0 / torch.sqrt(((x32 * x32).mean(-1) - mu * mu).clamp_min(0) + 1e-5)
    rstd64 = 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + 1e-5)
    return ((rstd32.double() - rstd64).abs() / rstd64).max().item()


def check_conditioning(device, mp, shift, rows=17):
    """a constant added to every feature of the three sources.  Asserted: the two-pass forms meet the rule at every shift, the folded
    forms meet it at shift 0 and are finite everywhere.  Recorded, not asserted: the folded forms' errors at shift > 0 beside cond =
    E[x^2] / var and beside the error of a plain fp32 one-pass restatement"""
    case = get_case(dims_of(rows), device, shift=shift)
    nA = case.dims[0]
    x = torch.stack([case.features(i, torch.float64).reshape(case.rows, -1) for i in range(nA)])
    cond = ((x * x).mean(-1) / x.var(-1, unbiased=False))
    table = {"cond_min": cond.min().item(), "cond_max": cond.max().item(), "one_pass_fp32_rstd": _one_pass_fp32(x)}
    print("shift", shift, "cond per row", cond.tolist())
    worst = {}
    for form in TWO_PASS:
        assert_vs_fp64(case, case.run(form, mp), worst, (form, "shift", shift))
    for k, v in worst.items():
        table["two_pass_" + k] = v
    for form in FOLDED:
        got = case.run(form, mp)
        for k in FLOAT_OUTS:
            assert torch.isfinite(got[k]).all(), (form, shift, k, "not finite")
        if shift == 0:
            assert_vs_fp64(case, got, {}, (form, "shift", shift))
        ok = True
        for k, (err, e32) in errors_vs_fp64(case, got).items():
            table[f"{form}_{k}"] = err
            table[f"{form}_{k}_bound"] = _bound(e32)
            ok = ok and err <= _bound(e32)
        table[f"{form}_within_bound"] = float(ok)
        print("shift", shift, form, {k: v for k, v in table.items() if k.startswith(form)})
    return table
