"""TEST INFRASTRUCTURE: policy inspection (csrc/policy_trace.hip, ops.policy_trace, DcntrlMAC.policy_trace / action_distribution) on
whatever library is active -- the host emulator in tests/test_emu_policy_trace.py, the gfx950 build in tests/test_gpu_policy_trace.py.

Ground truth: oracle.build_inputs_train / actor_logits / actor_evaluate / critic_value stepped over the S steps with the state carried,
in fp64 and in fp32.  Rule (tests/oracle_checks.py): error = max|got - ref64| / max|ref64| per tensor, net and step, bound =
max(1e-5, E32_FACTOR x the fp32 oracle's own error against fp64 on the same tensor at the same step).  The checks never touch
``L.use_library_for_tests``.  Each returns the worst errors."""
import functools

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log

TOL = 1e-5
M = 64
A = 32                                 # attention_dim of every case
# (nA, E, S, N, d, n_act) + options
KERNEL_CASES = [
    ((1, 1, 1, 2, 5, 5), {}),                                  # one chain, one step
    ((2, 2, 3, 3, 5, 5), {}),                                  # multi-step hand-off, partly filled tile
    ((1, 16, 2, 2, 5, 5), {}),                                 # exactly one full tile
    ((1, 17, 3, 2, 5, 5), {}),                                 # second tile holds a single valid chain
    ((1, 33, 2, 2, 5, 5), {}),                                 # three tiles
    ((5, 2, 5, 5, 7, 5), {}),                                  # agent count and feature width of the product, longer walk
    ((1, 2, 2, 4, 4, 16), {}),                                 # largest head
    ((1, 2, 2, 4, 5, 1), {}),                                  # smallest head
    ((1, 2, 2, 3, 5, 5), dict(latent=6)),                      # K-map edge: N w = 15 (history) and 18 (behaviour) end in padded k-tiles
    ((1, 2, 2, 3, 5, 5), dict(gat=False)),                     # absent source (attention)
    ((1, 2, 2, 3, 5, 5), dict(beh=False)),                     # absent source (behaviour)
    ((1, 2, 2, 3, 5, 5), dict(last_action=False, agent_id=False, last64=True)),   # no one-hots
    ((2, 2, 2, 3, 5, 5), dict(tanh=True)),                     # tanh trunk
]
# (attention_dim is 32 in every case, so N x 32 is always whole k-tiles: the ragged blocks are the history's and the behaviour latent's)
CASE_IDS = ["one_chain_one_step", "handoff", "full_tile", "one_past_tile", "three_tiles", "product_shape", "head16", "head1", "kmap_edge",
            "no_gat", "no_beh", "no_onehots", "tanh"]
OUTS = ("probs", "entropy", "greedy", "logp", "values", "h_actor", "h_critic")
FLOAT_OUTS = ("probs", "entropy", "logp", "values", "h_actor", "h_critic")
ALL_KEYS = OUTS + ("h_last_actor", "h_last_critic")


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _worse(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def assert_same_bits(a, b, what, keys=None):
    for k in (keys or sorted(set(a) & set(b))):
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def _args(device, nA, N, d, n_act, S, latent=8, gat=True, beh=True, last_action=True, agent_id=True, tanh=False, **kw):
    from iplan_amd.config import default_args
    return default_args("highway", use_cuda=torch.device(device).type == "cuda", max_vehicle_num=N, n_agents=nA, episode_limit=S,
                        n_actions=n_act, obs_shape_single=d, attention_dim=A, latent_dim=latent, GAT_enable=gat, Behavior_enable=beh,
                        GAT_use_behavior=gat and beh, obs_last_action=last_action, obs_agent_id=agent_id, use_ReLU=not tanh, **kw)


def make_mac(args, seed):
    """a DcntrlMAC whose parameters are spread out (the default initialisation leaves the heads near zero: every distribution would be
    uniform and every argmax a tie)"""
    from iplan_amd import synth
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    torch.manual_seed(seed)
    mac = DcntrlMAC(synth.make_scheme(args), {"agents": args.n_agents}, args)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in mac.agents + mac.critics:
            for p in m.parameters():
                p.add_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return mac


def _params(mac, dtype):
    conv = lambda m: {k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items()}  # noqa: E731
    return [conv(m) for m in mac.agents], [conv(m) for m in mac.critics]


def walk_reference(actor_p, critic_p, i, nA, fields, h0a, h0c, dtype, flags, use_relu=True):
    """agent i over the S steps of ``fields`` (history [E,S,N,d], att, beh, last [E,S] hot index or -1, avail [E,S,n_act] or None, actions
    [E,S]) from (h0a, h0c) [E,M] -> dict of probs [E,S,n_act], entropy / logp / values [E,S], h_actor / h_critic [E,S,M] in ``dtype``"""
    gat, beh, last_action, agent_id = flags
    hist = fields["history"].to(dtype)
    E, S, N = hist.shape[:3]
    n_act = actor_p["act.action_out.linear.bias"].shape[0]
    x = O.build_inputs_train(i, hist, fields["att"].to(dtype), fields["beh"].to(dtype), torch.zeros(E, S, n_act, dtype=dtype), nA, gat, beh)
    parts = [x[..., :x.shape[-1] - n_act - nA]]                               # the entity-major block; the one-hots as this trace defines them
    if last_action:
        last = fields["last"]
        oh = torch.zeros(E, S, n_act, dtype=dtype)
        oh.scatter_(-1, last.clamp_min(0).unsqueeze(-1), (last >= 0).to(dtype).unsqueeze(-1))
        parts.append(oh)
    if agent_id:
        idoh = torch.zeros(E, S, nA, dtype=dtype)
        idoh[..., i] = 1
        parts.append(idoh)
    x = torch.cat(parts, -1)
    ha, hc = h0a.to(dtype), h0c.to(dtype)
    out = {k: [] for k in FLOAT_OUTS}
    for s in range(S):
        av = None if fields["avail"] is None else fields["avail"][:, s]
        logits, ha_n = O.actor_logits(actor_p, x[:, s], ha, av, use_relu=use_relu)
        la = torch.log_softmax(logits, -1)
        lp, _ = O.actor_evaluate(actor_p, x[:, s], ha, fields["actions"][:, s], av, use_relu=use_relu)
        v, hc_n = O.critic_value(critic_p, x[:, s], hc, use_relu=use_relu)
        pr = la.exp()
        for k, t in (("probs", pr), ("entropy", -(pr * la.clamp_min(torch.finfo(dtype).min)).sum(-1)), ("logp", lp[:, 0]), ("values", v[:, 0]),
                     ("h_actor", ha_n), ("h_critic", hc_n)):
            out[k].append(t)
        ha, hc = ha_n, hc_n
    return {k: torch.stack(v, 1) for k, v in out.items()}


class Case:
    """a DcntrlMAC's arenas plus inputs that are strided views into larger episode-shaped buffers [E, S + 1, nA, width + padding]: T_phys
    = S + 1 and only the innermost block is packed.  ``poison``: every float outside the views (padding columns, physical step S, the
    hidden rows of steps > 0) is NaN, every integer outside them is junk; the views hold the same values either way."""
    PAD = 2                             # floats in front of every innermost block

    def __init__(self, dims, device, seed=0, poison=False, last64=False, **opt):
        nA, E, S, N, d, n_act = dims
        self.dims, self.device, self.opt, self.last64 = dims, device, opt, last64
        self.args = _args(device, nA, N, d, n_act, S, **opt)
        a = self.args
        self.flags = (a.GAT_enable, a.Behavior_enable, a.obs_last_action, a.obs_agent_id)
        self.mac = make_mac(a, 11 + seed)
        gen = torch.Generator().manual_seed(100 + seed + sum(dims))
        fill = float("nan") if poison else 0.25
        self.widths = [("history", d)] + ([("att", a.attention_dim)] if a.GAT_enable else []) + ([("beh", a.latent_dim)] if a.Behavior_enable else [])
        self.buf = {}
        for key, w in (("history", d), ("att", a.attention_dim), ("beh", a.latent_dim)):
            self.buf[key] = torch.full((E, S + 1, nA, N * w + 5), fill)
            vals = torch.rand(E, S, nA, N * w, generator=gen) * 2 - 1
            if key == "beh":
                vals = torch.softmax(vals.unflatten(-1, (N, w)) * 3, -1).flatten(-2)
            self.buf[key][:, :S, :, self.PAD:self.PAD + N * w] = vals
        for key in ("ha", "hc"):
            self.buf[key] = torch.full((E, S + 1, nA, M + 8), fill)
            self.buf[key][:, 0, :, 4:4 + M] = torch.randn(E, nA, M, generator=gen) * 0.3
        acts = torch.randint(0, n_act, (E, S, nA), generator=gen)
        self.buf["actions"] = torch.full((E, S + 1, nA, 2), 99 if poison else 0, dtype=torch.int64)
        self.buf["actions"][:, :S, :, 1] = acts
        self.buf["last"] = torch.full((E, S + 1, nA, 2), 77 if poison else 0, dtype=torch.int64 if last64 else torch.int32)
        self.buf["last"][:, 0, :, 0] = -1
        self.buf["last"][:, 1:S, :, 0] = acts[:, :S - 1].to(self.buf["last"].dtype)
        avail = (torch.rand(E, S, nA, n_act, generator=gen) < 0.7).int()
        avail.scatter_(-1, acts.unsqueeze(-1), 1)                                  # every recorded action is available
        avail[0, 0, 0] = 0
        avail[0, 0, 0, acts[0, 0, 0]] = 1                                          # a row with exactly one available action
        self.buf["avail"] = torch.full((E, S + 1, nA, n_act + 3), 5 if poison else 0, dtype=torch.int32)
        self.buf["avail"][:, :S, :, 1:1 + n_act] = avail
        self.order = torch.arange(E)
        self.upload()

    # ---- device side
    def upload(self, order=None):
        """(re)build the device buffers, optionally with the environments taken in ``order`` (a permutation or a subset)"""
        self.order = torch.arange(self.dims[1]) if order is None else torch.as_tensor(order)
        self.dbuf = {k: v[self.order].contiguous().to(self.device) for k, v in self.buf.items()}

    def operands(self, s0=0, s1=None):
        """what the ops over steps s0 .. s1 - 1 read, as views into the device buffers: (spec, the hidden rows of step 0 (actor, critic)
        [E, nA, M], avail [E, S', nA, n_act] int32, the recorded actions [E, S', nA] int64)"""
        nA, _, S, N, d, n_act = self.dims
        s1 = S if s1 is None else s1
        a, D = self.args, self.dbuf
        srcs = []
        for key, w in self.widths:
            v = D[key][:, s0:s1, :, self.PAD:self.PAD + N * w]                    # [E, S', nA, N w]
            assert v.untyped_storage().nbytes() > 4 * v.numel()                    # a view into a larger buffer, not a packed copy
            srcs.append((v, w, v.stride(2), v.stride(1)))
        last = D["last"][:, s0:s1, :, 0]
        spec = ops.AcFeatureSpec(N, srcs, n_actions=n_act if a.obs_last_action else 0, last_action=last if a.obs_last_action else None,
                                 la_strides=(last.stride(2), last.stride(1)), n_id=nA if a.obs_agent_id else 0, T=s1 - s0, T_phys=S + 1)
        assert spec.F == self.mac.input_shape
        return spec, (D["ha"][:, 0, :, 4:4 + M], D["hc"][:, 0, :, 4:4 + M]), D["avail"][:, s0:s1, :, 1:1 + n_act], D["actions"][:, s0:s1, :, 1]

    def run(self, s0=0, s1=None, hidden="buffer", avail=True, which=2, want=OUTS, packed=True, out=None, actions=True):
        """ops.policy_trace over steps s0 .. s1 - 1.  hidden: "buffer" (the hidden rows of step 0), None, or (actor, critic) [nA,E,M]"""
        nA, _, S, N, d, n_act = self.dims
        E = len(self.order)
        s1 = S if s1 is None else s1
        spec, (ha, hc), av, ac = self.operands(s0, s1)
        if isinstance(hidden, str):
            hs = (ha.stride(1), ha.stride(0))
        elif hidden is None:
            ha, hc, hs = None, None, (0, 0)
        else:
            ha, hc = hidden
            hs = (ha.stride(0), ha.stride(1))
        res = ops.policy_trace(self.mac.actor_arena, self.mac.critic_arena, which, spec, E, s1 - s0, nA, hidden0_actor=ha, hidden0_critic=hc, h_strides=hs,
                               avail=av if avail else None, avail_strides=(av.stride(2), av.stride(1)), actions_in=ac if actions else None,
                               act_strides=(ac.stride(2), ac.stride(1)), n_actions=n_act, want=want,
                               packed=self.mac.fc1_pack.get(spec) if packed else None, out=out)
        _sync(self.device)
        return res

    # ---- reference side
    def fields(self, i):
        nA, E, S, N, d, n_act = self.dims
        a = self.args
        f = {}
        for key, w in (("history", d), ("att", a.attention_dim), ("beh", a.latent_dim)):
            f[key] = self.buf[key][:, :S, i, self.PAD:self.PAD + N * w].unflatten(-1, (N, w))
        f["last"] = self.buf["last"][:, :S, i, 0].long()
        f["avail"] = self.buf["avail"][:, :S, i, 1:1 + n_act]
        f["actions"] = self.buf["actions"][:, :S, i, 1]
        return f

    def reference(self, dtype, hidden=True, avail=True):
        """dict of [nA, E, S, ...] tensors in ``dtype`` (computed once per variant, never modified)"""
        return _reference(self, dtype, hidden, avail)


@functools.lru_cache(maxsize=None)
def _reference(case, dtype, hidden, avail):
    nA, E = case.dims[:2]
    ap, cp = _params(case.mac, dtype)
    res = []
    for i in range(nA):
        f = case.fields(i)
        if not avail:
            f["avail"] = None
        h0a = case.buf["ha"][:, 0, i, 4:4 + M] if hidden else torch.zeros(E, M)
        h0c = case.buf["hc"][:, 0, i, 4:4 + M] if hidden else torch.zeros(E, M)
        res.append(walk_reference(ap[i], cp[i], i, nA, f, h0a, h0c, dtype, case.flags, use_relu=case.args.use_ReLU))
    return {k: torch.stack([r[k] for r in res]) for k in FLOAT_OUTS}


@functools.lru_cache(maxsize=None)
def get_case(dims, device, opt=(), seed=0, poison=False):
    return Case(dims, device, seed=seed, poison=poison, **dict(opt))


def lowest_argmax(probs):
    n = probs.shape[-1]
    idx = torch.arange(n, device=probs.device).expand_as(probs)
    return torch.where(probs == probs.max(-1, keepdim=True).values, idx, torch.full_like(idx, n)).min(-1).values


def assert_vs_fp64(got, r64, r32, worst, what, keys=FLOAT_OUTS, scale=1.0, other=None):
    """every tensor of ``got`` ([nA, E, S, ...]) at every net and step under the rule; ``other``: a second result compared with ``got``
    under ``scale`` x the bound instead (the triangle inequality over two implementations that each meet the bound)"""
    for k in keys:
        if k not in got:
            continue
        g = got[k].cpu()
        nA, _, S = g.shape[:3]
        for i in range(nA):
            for s in range(S):
                ref = r64[k][i, :, s]
                e32 = _grad_err(r32[k][i, :, s], ref)
                err = _grad_err(g[i, :, s], ref)
                print(what, k, "net", i, "step", s, "err", err, "e32", e32)
                _worse(worst, k, err)
                _worse(worst, k + "_e32", e32)
                assert err <= _bound(e32), (what, k, i, s, err, e32)
                if other is not None:
                    diff = (other[k].cpu()[i, :, s].double() - g[i, :, s].double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)
                    _worse(worst, k + "_between", diff)
                    assert diff <= scale * _bound(e32), (what, k, "between the two", i, s, diff, e32)


def assert_head_properties(case, got, what):
    n_act = case.dims[5]
    avail = case.buf["avail"][case.order][:, :case.dims[2], :, 1:1 + n_act].permute(2, 0, 1, 3)       # [nA, E, S, n_act]
    probs = got["probs"].cpu()
    assert torch.equal(probs[avail == 0], torch.zeros_like(probs[avail == 0])), (what, "an unavailable action has a non-zero probability")
    assert torch.equal(got["greedy"].cpu(), lowest_argmax(probs)), (what, "greedy is not the lowest-index argmax of the returned probs")
    assert got["greedy"].dtype == torch.int64


# ------------------------------------------------------------------------------------------------ the kernels alone
def check_kernel(device, dims, opt):
    """1: every output at every step against fp64; exact zeros at unavailable actions; greedy == argmax of the kernel's own probs"""
    case = get_case(dims, device, tuple(sorted(opt.items())))
    worst = {}
    got = case.run()
    assert_vs_fp64(got, case.reference(torch.float64), case.reference(torch.float32), worst, (dims, opt))
    assert_head_properties(case, got, (dims, opt))
    assert_same_bits({"h_last_actor": got["h_actor"][:, :, -1], "h_last_critic": got["h_critic"][:, :, -1]}, got, "last state")
    return worst


def check_step_splitting(device, dims=(5, 2, 5, 5, 7, 5)):
    """2: one trace over S = 5 == steps 0-1 then 2-4 with the returned state fed in == five single steps, bit for bit"""
    case = get_case(dims, device)
    S = dims[2]
    full = case.run()
    for cuts in ((0, 2, S), tuple(range(S + 1))):
        hidden = "buffer"
        for s0, s1 in zip(cuts[:-1], cuts[1:]):
            part = case.run(s0, s1, hidden=hidden)
            for k in OUTS:
                assert torch.equal(_bits(part[k]), _bits(full[k][:, :, s0:s1])), (cuts, s0, k)
            hidden = (part["h_last_actor"], part["h_last_critic"])
        assert_same_bits(part, full, cuts, ("h_last_actor", "h_last_critic"))
    return {}


def check_tiling(device, dims=(1, 17, 3, 2, 5, 5)):
    """3: every chain of E = 17 alone (E = 1) and the batch in reversed environment order give the chain's bits"""
    case = get_case(dims, device)
    E = dims[1]
    full = case.run()
    try:
        for e in range(E):
            case.upload([e])
            one = case.run()
            for k in ALL_KEYS:
                assert torch.equal(_bits(one[k][:, 0]), _bits(full[k][:, e])), (e, k, "alone")
        rev = list(range(E - 1, -1, -1))
        case.upload(rev)
        back = case.run()
        for k in ALL_KEYS:
            assert torch.equal(_bits(back[k].flip(1)), _bits(full[k])), (k, "reversed")
    finally:
        case.upload()
    return {}


def _sentinels(case, device, shift=0.0):
    nA, E, S, _, _, n_act = case.dims
    shapes = dict(probs=(nA, E, S, n_act), entropy=(nA, E, S), greedy=(nA, E, S), logp=(nA, E, S), values=(nA, E, S), h_actor=(nA, E, S, M),
                  h_critic=(nA, E, S, M), h_last_actor=(nA, E, M), h_last_critic=(nA, E, M))
    bufs = {}
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        if k == "greedy":
            sent = torch.arange(n + 64, dtype=torch.int64) * 7 + 1000
        else:
            sent = 0.5 + shift + (torch.arange(n + 64, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        bufs[k] = (sent, buf, buf[32:32 + n].view(shape))
    return bufs


def check_sentinel(device, dims=(2, 2, 3, 3, 5, 5)):
    """4: outputs carved out of sentinel-filled buffers: nothing outside the owned region is written, every owned element is, and an
    output that was not asked for is neither allocated nor written"""
    case = get_case(dims, device)
    ref = case.run()
    for which, wanted in ((2, OUTS), (2, ("probs", "values")), (1, ("values",)), (0, ("greedy", "h_actor"))):
        bufs = _sentinels(case, device)
        got = case.run(which=which, want=wanted, out={k: v[2] for k, v in bufs.items()})
        owned = set(wanted) | {"h_last_" + n for n, on in (("actor", which != 1), ("critic", which != 0)) if on}
        assert set(got) == owned, (which, wanted, sorted(got))
        for k, (sent, buf, view) in bufs.items():
            host = buf.cpu()
            if k not in owned:
                assert torch.equal(host, sent), (k, "was not asked for and was written")
                continue
            assert got[k].data_ptr() == view.data_ptr()
            assert torch.equal(_bits(view), _bits(ref[k])), (k, "differs inside a padded buffer")
            n = view.numel()
            assert torch.equal(host[:32], sent[:32]) and torch.equal(host[32 + n:], sent[32 + n:]), (k, "an element outside the owned region was written")
    b2 = _sentinels(case, device, 0.25)                      # every owned element is written: a second, shifted sentinel ends the same
    case.run(out={k: v[2] for k, v in b2.items()})
    for k in ALL_KEYS:
        assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (k, "an owned element was left unwritten")
    return {}


def check_poison(device, dims=(2, 2, 3, 3, 5, 5)):
    """5: NaN in every float the views do not own (padding columns, physical step S, hidden rows of other steps): finite, same bits"""
    clean, dirty = get_case(dims, device), get_case(dims, device, poison=True)
    for k in ("history", "att", "beh", "ha", "hc"):
        assert torch.isnan(dirty.buf[k]).any() and not torch.isnan(clean.buf[k]).any()
    for packed in (True, False):
        a, b = clean.run(packed=packed), dirty.run(packed=packed)
        for k in ALL_KEYS:
            assert k == "greedy" or torch.isfinite(b[k]).all(), (k, "not finite")
            assert torch.equal(_bits(a[k]), _bits(b[k])), (k, "read something outside its views")
    return {}


def check_optional_operands(device, dims=(2, 2, 3, 3, 5, 5)):
    """6: hidden0 null == zeros, avail null == all ones, `which` 0 / 1 / 2 share bits, packed == in place (the notes claim the same
    bits: the operands hold the same values and meet the same instructions)"""
    case = get_case(dims, device)
    nA, E = dims[:2]
    worst = {}
    base = case.run()
    none = case.run(hidden=None)
    assert_vs_fp64(none, case.reference(torch.float64, hidden=False), case.reference(torch.float32, hidden=False), worst, "hidden0 null")
    z = torch.zeros(nA, E, M, device=device)
    assert_same_bits(none, case.run(hidden=(z, z.clone())), "hidden0 null != explicit zeros", ALL_KEYS)
    free = case.run(avail=False)
    assert_vs_fp64(free, case.reference(torch.float64, avail=False), case.reference(torch.float32, avail=False), worst, "avail null")
    keep = case.buf["avail"].clone()
    try:
        case.buf["avail"].fill_(1)
        case.upload()
        assert_same_bits(free, case.run(), "avail null != all ones", ALL_KEYS)
    finally:
        case.buf["avail"].copy_(keep)
        case.upload()
    actor, critic = case.run(which=0), case.run(which=1)
    assert set(actor) == {"probs", "entropy", "greedy", "logp", "h_actor", "h_last_actor"} and set(critic) == {"values", "h_critic", "h_last_critic"}
    assert_same_bits(actor, base, "which = 0")
    assert_same_bits(critic, base, "which = 1")
    inplace = case.run(packed=False)
    assert_vs_fp64(inplace, case.reference(torch.float64), case.reference(torch.float32), worst, "fc1 operands in place")
    assert_same_bits(inplace, base, "packed != in place", ALL_KEYS)
    return worst


def check_agrees_with_ac_forward(device, dims=(2, 17, 1, 3, 5, 5)):
    """7: an S = 1 trace and ops.ac_forward(ksplit=1, mode=2) on the same rows: each within its bound of fp64, their difference within
    the sum of the two bounds"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    worst = {}
    tr = case.run()
    D, a = case.dbuf, case.args
    srcs = []
    for key, w in case.widths:
        v = D[key][:, :S, :, case.PAD:case.PAD + N * w]
        srcs.append((v, w, v.stride(2), v.stride(1)))
    last = D["last"][:, :S, :, 0]
    spec = ops.AcFeatureSpec(N, srcs, n_actions=n_act, last_action=last, la_strides=(last.stride(2), last.stride(1)), n_id=nA, T=S, T_phys=S + 1)
    ha, hc = D["ha"][:, :, :, 4:4 + M], D["hc"][:, :, :, 4:4 + M]                # [E, S + 1, nA, M]: physical rows e (S + 1) + s
    av, ac = D["avail"][:, :, :, 1:1 + n_act], D["actions"][:, :, :, 1]
    one = ops.ac_forward(case.mac.actor_arena, case.mac.critic_arena, 2, spec, E * S, nA, h_actor=ha, h_critic=hc, h_strides=(ha.stride(2), ha.stride(1)),
                         avail=av, avail_strides=(av.stride(2), av.stride(1)), mode=2, actions_in=ac, act_strides=(ac.stride(2), ac.stride(1)),
                         n_actions=n_act, ksplit=1, want_probs=True, want_entropy=True)
    _sync(device)
    step = {k: one[k].reshape(nA, E, S, *one[k].shape[2:]) for k in FLOAT_OUTS}
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    assert_vs_fp64(step, r64, r32, worst, "ac_forward")
    assert_vs_fp64(tr, r64, r32, worst, "trace", scale=2.0, other=step)
    return worst


def check_one_categorical(device, n_act):
    """7b: the four inspection ops share one statement of the masked categorical (csrc/ac_categorical.h) behind the same forward
    arithmetic, so on the same rows from the same given state -- nA = 2, E = 2, S = 1, N = 3 -- they give the same BITS: ops.policy_trace,
    ops.saliency(want=("y",)), ops.policy_knockout(want=("base",)) and ops.policy_knockout_trace(want=("base",), H = D = 1).  n_act = 3
    leaves a lane's four-slot group partly empty.  Row (e 0, agent 0) has every action available, (0, 1) a single one, (1, 0) none (the
    uniform distribution), (1, 1) whatever the case drew.  Compared pairwise, with the recorded action as a*: logp and values of all
    four, probs and greedy of the three that return them, target_action of the three that return it; with a* = the row's own argmax:
    logp and target_action of the three that take such a target, and that target against policy_trace's greedy."""
    dims = (2, 2, 1, 3, 5, n_act)
    nA, E, S, N = dims[:4]
    case = Case(dims, device, seed=3)                                              # (not the shared one: its avail is edited)
    acts = case.buf["actions"][:, :S, :, 1]
    av = case.buf["avail"][:, :S, :, 1:1 + n_act]
    av[0, 0, 0] = 1
    av[0, 0, 1] = 0
    av[0, 0, 1, acts[0, 0, 1]] = 1
    av[1, 0, 0] = 0
    case.upload()
    mac = case.mac
    spec, (ha, hc), avail, actions = case.operands()
    packed = mac.fc1_pack.get(spec)
    hs2, hs3 = (ha.stride(1), ha.stride(0)), (ha.stride(1), ha.stride(0), 0)
    by_row = lambda t: (t.stride(2), t.stride(1))                                  # noqa: E731
    esn = lambda t: (t.stride(2), t.stride(0), t.stride(1))                        # noqa: E731
    greedy_tgt = torch.full_like(case.dbuf["actions"], -1)[:, :S, :, 1]               # (addressed by physical row, like the recorded ones)
    got = {}
    for tag, tgt in (("recorded", actions), ("greedy", greedy_tgt)):
        res = {"trace": case.run(want=("probs", "logp", "greedy", "values"))} if tag == "recorded" else {}
        res["saliency"] = ops.saliency(mac.actor_arena, mac.critic_arena, 2, spec, E, S, nA, h_actor=ha, h_critic=hc, h_strides=hs3, avail=avail,
                                       avail_strides=esn(avail), target=tgt, target_strides=esn(tgt), n_actions=n_act, want=("y",), packed=packed)
        res["knockout"] = ops.policy_knockout(mac.actor_arena, mac.critic_arena, 2, spec, E, S, nA, [1], h_actor=ha, h_critic=hc, h_strides=hs3,
                                              avail=avail, avail_strides=esn(avail), target=tgt, target_strides=esn(tgt), n_actions=n_act,
                                              want=("base",), packed=packed)
        res["knockout_trace"] = ops.policy_knockout_trace(mac.actor_arena, mac.critic_arena, 2, spec, E, S, S, nA, [1], hidden0_actor=ha,
                                                          hidden0_critic=hc, h_strides=hs2, avail=avail, avail_strides=by_row(avail), target=tgt,
                                                          target_strides=by_row(tgt), n_actions=n_act, want=("base",), packed=packed)
        _sync(device)
        got[tag] = res
        for k, n_ops in (("logp", 3), ("values", 3), ("probs", 2), ("greedy", 2), ("target_action", 3)):
            have = [n for n in sorted(res) if k in res[n]]
            assert len(have) == n_ops + (tag == "recorded" and k != "target_action"), (tag, k, have)
            for n in have[1:]:
                assert torch.equal(_bits(res[have[0]][k]), _bits(res[n][k])), (tag, k, have[0], n, "bits differ")
    rec, gr = got["recorded"], got["greedy"]
    assert torch.equal(rec["saliency"]["target_action"].cpu(), acts.permute(2, 0, 1))
    assert torch.equal(gr["saliency"]["target_action"], rec["trace"]["greedy"]), "a* = the row's argmax"
    # the rows are what the docstring says they are
    p = rec["trace"]["probs"].cpu()                                                # [nA, E, S, n_act]
    assert (p[0, 0, 0] > 0).all() and (p[1, 0, 0] > 0).sum() == 1 and torch.equal(p[0, 1, 0], torch.full((n_act,), 1.0 / n_act))
    return {}


def check_repeatable(device, reps, dims=(2, 2, 3, 3, 5, 5)):
    """8: ``reps`` launches on the same inputs: identical bits"""
    case = get_case(dims, device)
    first = case.run()
    for _ in range(reps - 1):
        assert_same_bits(case.run(), first, "repeat", ALL_KEYS)
    return {}


def _codes():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "iplan_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"(IPLAN_E\w+)\s*=\s*(-?\d+)", text)}
    return vals["IPLAN_EINVAL"]


def assert_out_refused(call, bufs, keys):
    """``call(out)`` raises AssertionError when ``out[k]``, k in ``keys``, has the wrong shape, the wrong dtype or is not contiguous, the
    other destinations being the good views of the sentinel-filled ``bufs`` (which the caller then finds untouched: nothing was launched)"""
    good = {k: v[2] for k, v in bufs.items()}
    for k in keys:
        t = good[k]
        assert t.numel() > 1
        strided = torch.zeros(*t.shape, 2, dtype=t.dtype, device=t.device)[..., 0]
        assert strided.shape == t.shape and not strided.is_contiguous()
        for what, bad in (("shape", t.unsqueeze(0)), ("dtype", t.to(torch.float64)), ("not contiguous", strided)):
            try:
                call({**good, k: bad})
            except AssertionError:
                pass
            else:
                raise AssertionError(f"out[{k!r}] of the wrong {what} was not refused")


def check_bad_arguments(device, dims=(2, 2, 3, 3, 5, 5)):
    """9: each invalid descriptor is refused by the host-side check with IPLAN_EINVAL and a message; an ``out=`` destination of the wrong
    shape or dtype, or a non-contiguous one, makes ops.policy_trace raise AssertionError; nothing is launched, so the sentinel-filled
    outputs of the descriptor stay as they were"""
    case = get_case(dims, device)
    nA, E, S, N, d, n_act = dims
    good = case.run()
    lib = ops._lib(None)
    D = case.dbuf
    srcs = []
    for key, w in case.widths:
        v = D[key][:, :S, :, case.PAD:case.PAD + N * w]
        srcs.append((v, w, v.stride(2), v.stride(1)))
    last = D["last"][:, :S, :, 0]
    spec = ops.AcFeatureSpec(N, srcs, n_actions=n_act, last_action=last, la_strides=(last.stride(2), last.stride(1)), n_id=nA, T=S, T_phys=S + 1)
    av, ac = D["avail"][:, :S, :, 1:1 + n_act], D["actions"][:, :S, :, 1]
    bufs = _sentinels(case, device)
    a, res, keep = ops.policy_trace_args(case.mac.actor_arena, case.mac.critic_arena, 2, spec, E, S, nA, avail=av, avail_strides=(av.stride(2), av.stride(1)),
                                         actions_in=ac, act_strides=(ac.stride(2), ac.stride(1)), n_actions=n_act, want=OUTS,
                                         out={k: v[2] for k, v in bufs.items()})
    EINVAL = _codes()
    fn = lib.c.iplan_ac_trace

    def refused(args_ref, **fields):
        keep_f = {}
        for k, v in fields.items():
            obj, name = (a, k) if "." not in k else (getattr(a, k.split(".")[0]), k.split(".")[1])
            keep_f[k] = (obj, name, getattr(obj, name))
            setattr(obj, name, v)
        rc = fn(args_ref, L.C.c_void_p(0))
        msg = lib.c.iplan_last_error().decode()
        for obj, name, v in keep_f.values():
            setattr(obj, name, v)
        assert rc == EINVAL and "iplan_ac_trace" in msg, (fields, rc, msg)

    refused(None)
    ref = L.C.byref(a)
    refused(ref, S=0)
    refused(ref, E=0)
    refused(ref, **{"actor.n_out": 0})
    refused(ref, **{"actor.n_out": 17})
    refused(ref, which=3)
    refused(ref, gi=None)
    refused(ref, actions_in=None)                             # logp is asked for
    assert_out_refused(lambda out: ops.policy_trace(case.mac.actor_arena, case.mac.critic_arena, 2, spec, E, S, nA, avail=av,
                                                    avail_strides=(av.stride(2), av.stride(1)), actions_in=ac, act_strides=(ac.stride(2), ac.stride(1)),
                                                    n_actions=n_act, want=OUTS, out=out), bufs, ("probs", "greedy", "h_last_critic"))
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(buf.cpu(), sent), (k, "a refused call wrote an output")
    again = case.run()
    assert_same_bits(again, good, "after the refusals", ALL_KEYS)
    del keep, res
    return {}


# ------------------------------------------------------------------------------------------------ the methods
def _e2e_args(device, **kw):
    from iplan_amd.config import default_args
    base = dict(use_cuda=torch.device(device).type == "cuda", max_vehicle_num=5, n_agents=2, episode_limit=5, batch_size_run=3, max_history_len=3,
                pred_batch_size=6, pred_length=2, buffer_size=4, batch_size=3, ppo_epoch=2)
    base.update(kw)
    return default_args("highway", **base)


def _method_reference(mac, f, dtype, h0a, h0c, t0=0, S=None):
    """the fp64 / fp32 walk of every agent over steps t0 .. t0 + S - 1 of the episode fields ``f`` ([E, T1, nA, ...]), the last action of
    step t being the recorded action of t - 1 (none at t = 0) -> dict of [nA, E, S, ...]"""
    a = mac.args
    nA = a.n_agents
    T1 = f["history"].shape[1]
    S = T1 - t0 if S is None else S
    ap, cp = _params(mac, dtype)
    acts = f["actions"][..., 0]
    last_all = torch.cat([torch.full_like(acts[:, :1], -1), acts[:, :-1]], 1)
    sl = slice(t0, t0 + S)
    res = []
    for i in range(nA):
        fi = dict(history=f["history"][:, sl, i], att=f["attention_latent"][:, sl, i], beh=f["behavior_latent"][:, sl, i], last=last_all[:, sl, i],
                  avail=f["avail_actions"][:, sl, i], actions=acts[:, sl, i])
        res.append(walk_reference(ap[i], cp[i], i, nA, fi, h0a[:, i], h0c[:, i], dtype, (a.GAT_enable, a.Behavior_enable, a.obs_last_action, a.obs_agent_id),
                                  use_relu=a.use_ReLU))
    return {k: torch.stack([r[k] for r in res]) for k in FLOAT_OUTS}


def _stats_of(ref, greedy, f, dtype=torch.float64):
    """[nA, S, 6] in fp64 from per-row results [nA, E, S, ..]: sums over the environments with weight filled"""
    w = f["filled"][:, :, 0].to(dtype)                                           # [E, S]
    hit = (greedy == f["actions"][..., 0].permute(2, 0, 1)).to(dtype)
    cols = torch.stack([torch.ones_like(hit), ref["entropy"].to(dtype), hit, ref["logp"].to(dtype), ref["values"].to(dtype),
                        ref["probs"].to(dtype).max(-1).values], -1)
    return (cols * w[None, :, :, None]).sum(1)


def _to_ref_shape(got):
    """the methods' [E, S, nA, ...] -> [nA, E, S, ...]"""
    out = {}
    for k, v in got.items():
        v = torch.as_tensor(v)
        if k in FLOAT_OUTS and v.dim() >= (4 if k.startswith("h_") else 3):     # (h_* [E, nA, M] without return_hidden has no step axis)
            out[k] = v.permute(2, 0, 1, *range(3, v.dim()))
    return out


def check_methods(device, tmp_path, E=4):
    """10: policy_trace / action_distribution on a loaded checkpoint, numpy-backed and device-backed batches: shapes, dtypes, devices,
    values and the six sums against fp64.
    The sums are compared relative to EACH SUM, and the rule bounds a row's error by the scale of its tensor, not by the row's own size:
    a sum is held to the rule only where it is about as large as its terms.  Entropy, logp, the largest probability and the counts have
    one sign; the values do not, so the critics' output bias is moved away from zero (values around +4 instead of around 0) and at
    least two environments stay filled at every step -- otherwise a step's value sum can be one small number or a cancelling pair, and
    its error relative to itself says nothing about the kernels (the per-row values are held to the rule in every kernel case)."""
    from iplan_amd import synth
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    args = _e2e_args(device)
    src = make_mac(args, 23)
    with torch.no_grad():
        for c in src.critics:
            c.v_out.bias.add_(4.0)
    src.save_models(str(tmp_path))
    mac = DcntrlMAC(synth.make_scheme(args), {"agents": args.n_agents}, args)
    mac.load_models([str(tmp_path)])
    nA, n_act, T1 = args.n_agents, args.n_actions, args.episode_limit + 1
    f = synth.make_episode_fields(args, E, seed=5, terminated_p=0.2)
    f["avail_actions"].scatter_(-1, f["actions"], 1)
    f["filled"][1, 4:] = 0
    f["filled"][3, 2:] = 0
    np_batch = synth.DictBatch({k: v.numpy() for k, v in f.items()}, E, T1)
    dev_batch = synth.DictBatch(f, E, T1).to(device)
    before = (mac.actor_arena.data.clone(), mac.critic_arena.data.clone(), {k: v.clone() for k, v in dev_batch.data.items()})
    states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None)
    mac.hidden_states = "untouched"
    worst = {}
    got_np = mac.policy_trace(np_batch, return_hidden=True)
    got = mac.policy_trace(dev_batch, return_hidden=True)
    last = mac.policy_trace(dev_batch)
    _sync(device)
    shapes = dict(probs=(E, T1, nA, n_act), entropy=(E, T1, nA), logp=(E, T1, nA), values=(E, T1, nA), greedy=(E, T1, nA), h_actor=(E, T1, nA, M),
                  h_critic=(E, T1, nA, M), stats=(nA, T1, 6))
    assert set(got) == set(shapes) == set(got_np)
    for k, shape in shapes.items():
        assert isinstance(got_np[k], np.ndarray) and got_np[k].shape == shape, (k, got_np[k].shape)
        assert torch.is_tensor(got[k]) and got[k].shape == shape and got[k].device.type == torch.device(device).type, (k, got[k].shape)
        want_dtype = torch.float64 if k == "stats" else (torch.int64 if k == "greedy" else torch.float32)
        assert got[k].dtype == want_dtype and torch.as_tensor(got_np[k]).dtype == want_dtype, k
        assert np.array_equal(got[k].cpu().numpy(), got_np[k]), (k, "numpy-backed and device-backed batches differ")
    for k in ("h_actor", "h_critic"):
        assert last[k].shape == (E, nA, M) and torch.equal(last[k], got[k][:, -1]), k
    h0a, h0c = f["rnn_states_actors"][:, 0], f["rnn_states_critics"][:, 0]
    r64, r32 = (_method_reference(mac, f, dt, h0a, h0c) for dt in (torch.float64, torch.float32))
    assert_vs_fp64(_to_ref_shape(got), r64, r32, worst, "policy_trace")
    g = got["greedy"].permute(2, 0, 1).cpu()
    assert torch.equal(g, lowest_argmax(got["probs"].permute(2, 0, 1, 3).cpu()))
    # the six sums relative to each sum; the fp32 oracle's own sums give e32.  The hit column is taken with the kernel's own greedy
    # actions (an index is not a rounded quantity); everything else comes from the oracle.
    s64, s32 = _stats_of(r64, g, f), _stats_of(r32, g, f)
    st = got["stats"].cpu()
    for i in range(nA):
        for s in range(T1):
            for c in range(6):
                ref = s64[i, s, c:c + 1]
                if ref.abs().max() == 0:
                    assert st[i, s, c] == 0, ("stat", c, i, s)
                    continue
                e32, err = _grad_err(s32[i, s, c:c + 1], ref), _grad_err(st[i, s, c:c + 1], ref)
                _worse(worst, f"stat{c}", err)
                assert err <= _bound(e32), ("stat", c, i, s, err, e32)
    assert torch.equal(st[..., 0], f["filled"][:, :, 0].sum(0).double().expand(nA, T1))
    # hidden0 variants and the nets one at a time
    zeros = mac.policy_trace(dev_batch, hidden0="zeros", want=("values", "logp"))
    z = torch.zeros(E, nA, M)
    pair = mac.policy_trace(dev_batch, hidden0=(z, z.numpy()), want=("values", "logp"))
    assert set(zeros) == {"values", "logp", "h_actor", "h_critic"}
    assert_same_bits(zeros, pair, "hidden0 zeros != a pair of zero tensors")
    zr64, zr32 = (_method_reference(mac, f, dt, z, z) for dt in (torch.float64, torch.float32))
    assert_vs_fp64(_to_ref_shape(zeros), zr64, zr32, worst, "hidden0 zeros")
    only_a, only_c = mac.policy_trace(dev_batch, which="actor", want=("probs", "values")), mac.policy_trace(dev_batch, which="critic", want=("probs", "values"))
    assert set(only_a) == {"probs", "h_actor"} and set(only_c) == {"values", "h_critic"}
    assert_same_bits(only_a, got, "which = actor", ("probs",))
    assert_same_bits(only_c, got, "which = critic", ("values",))
    # one step from the stored states
    for t_ep in (0, 2):
        d_np, d_dev = mac.action_distribution(np_batch, t_ep), mac.action_distribution(dev_batch, t_ep)
        _sync(device)
        d64, d32 = (_method_reference(mac, f, dt, f["rnn_states_actors"][:, t_ep], f["rnn_states_critics"][:, t_ep], t_ep, 1) for dt in (torch.float64, torch.float32))
        for k, shape in (("probs", (E, nA, n_act)), ("greedy", (E, nA)), ("entropy", (E, nA)), ("values", (E, nA))):
            assert isinstance(d_np[k], np.ndarray) and d_np[k].shape == shape and torch.is_tensor(d_dev[k]) and d_dev[k].shape == shape, (k, t_ep)
            assert np.array_equal(d_np[k], d_dev[k].cpu().numpy()), (k, t_ep)
        assert set(d_dev) == {"probs", "greedy", "entropy", "values"}
        step = {k: d_dev[k].transpose(0, 1).unsqueeze(2) for k in ("probs", "entropy", "values")}
        assert_vs_fp64(step, d64, d32, worst, f"action_distribution t_ep={t_ep}", keys=("probs", "entropy", "values"))
        assert torch.equal(d_dev["greedy"].cpu(), lowest_argmax(d_dev["probs"].cpu()))
    # nothing was drawn, nothing was touched
    assert torch.equal(torch.get_rng_state(), states[0])
    if states[1] is not None:
        assert torch.equal(torch.cuda.get_rng_state(), states[1])
    assert mac.hidden_states == "untouched"
    assert torch.equal(mac.actor_arena.data, before[0]) and torch.equal(mac.critic_arena.data, before[1])
    for k, v in before[2].items():
        assert torch.equal(dev_batch.data[k], v), (k, "the batch was written")
    return worst


def check_replays_rollout(device, E=2, N=7, T=6):
    """11: policy_trace on a device-resident rollout's own batch: the traced state after step s against rnn_states_*[:, s + 1], the
    traced values / logp against what the rollout's launches returned, each within the sum of the two kernels' bounds against the fp64
    walk.
    As in check_methods the critics' output bias is moved away from zero (values around +4 instead of around 0).  The rule divides a
    step's error by the largest |value| of that step, here over E = 2 environments, while the rounding error of a value is set by the
    size of the 64 products the head sums (sum |w_j x_j| ~ 15 with these weights, so ~ 2e-6 absolute in any fp32 implementation).  With
    values spread around zero both environments of a step can land near it -- 0.29 and -0.26 at one step of this rollout, where the fp32
    oracle itself is 4e-6 and the one-step kernel 8e-6 away from fp64 by that measure -- and the figure then measures the draw, not the
    kernels.  With the bias moved the divisor is the size of what is summed at every step; bounds and cases are unchanged."""
    from iplan_amd.harness import SyntheticLoop
    from tests.attention_checks import _gumbel
    args = _e2e_args(device, max_vehicle_num=N, episode_limit=T, batch_size_run=E)
    nA = args.n_agents
    loop = SyntheticLoop(args, E, seed=4, device=device)
    gen = torch.Generator().manual_seed(15)
    with torch.no_grad():
        for m in loop.mac.agents + loop.mac.critics:
            for p in m.parameters():
                p.add_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
        for c in loop.mac.critics:
            c.v_out.bias.add_(4.0)
    noise = _gumbel(gen, T + 1, nA, E, N, N - 1, 2).to(device)
    q_all = -torch.log(torch.rand(T, nA, E, args.n_actions, generator=gen).clamp_min(1e-20)).to(device)
    recorded = {}
    select = loop.mac.select_actions_ippo

    def recording(ep_batch, t_ep, *a, **kw):                                    # what the rollout's action selection returns and drops
        out = select(ep_batch, t_ep, *a, **kw)
        recorded[t_ep] = (out["values"], out["logp"]) if isinstance(out, dict) else (out[0].t(), torch.stack([lp[:, 0] for lp in out[2]]))
        return out
    loop.mac.select_actions_ippo = recording
    batch = loop.new_batch()
    with torch.no_grad():
        loop._rollout_body(loop.obs_sets[0], batch, noise=noise, q_all=q_all)
    _sync(device)
    loop.mac.select_actions_ippo = select
    assert sorted(recorded) == list(range(T))
    got = loop.mac.policy_trace(batch, return_hidden=True)
    _sync(device)
    f = {k: v.cpu() for k, v in batch.data.items()}
    z = torch.zeros(E, nA, M)
    r64, r32 = (_method_reference(loop.mac, f, dt, z, z, 0, T) for dt in (torch.float64, torch.float32))
    roll = dict(h_actor=f["rnn_states_actors"][:, 1:T + 1].permute(2, 0, 1, 3), h_critic=f["rnn_states_critics"][:, 1:T + 1].permute(2, 0, 1, 3),
                values=torch.stack([recorded[t][0].cpu() for t in range(T)], -1), logp=torch.stack([recorded[t][1].cpu() for t in range(T)], -1))
    assert roll["h_actor"].abs().sum() > 0 and roll["values"].shape == (nA, E, T)
    traced = {k: v[:, :, :T] for k, v in _to_ref_shape(got).items()}
    worst = {}
    keys = ("h_actor", "h_critic", "values", "logp")
    assert_vs_fp64(roll, r64, r32, worst, "rollout", keys=keys)
    assert_vs_fp64(traced, r64, r32, worst, "trace of the rollout", keys=keys, scale=2.0, other=roll)
    return worst


def check_train_unaffected(device):
    """12: IPPOLearner.train gives the same parameters, bit for bit, whether or not a policy_trace ran between the insert and the train;
    the trace leaves the generators and mac.hidden_states alone"""
    from iplan_amd import synth
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    from iplan_amd.learners.ippo_learner import IPPOLearner
    from tests.oracle_checks import _fields
    args = _e2e_args(device, episode_limit=9)
    results = []
    for with_trace in (False, True):
        torch.manual_seed(6)
        scheme = synth.make_scheme(args)
        mac = DcntrlMAC(scheme, {"agents": args.n_agents}, args)
        learner = IPPOLearner(mac, scheme, _Log(), args)
        E = args.buffer_size
        _, batch = _fields(args, E, 7, 0.15, device)
        learner.batch_size_run = E
        learner.insert_episode_batch(batch)
        torch.manual_seed(83)
        if with_trace:
            states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None)
            hidden = mac.hidden_states
            tr = mac.policy_trace(batch)
            assert torch.isfinite(tr["stats"]).all() and torch.isfinite(tr["probs"]).all()
            assert torch.equal(torch.get_rng_state(), states[0]) and mac.hidden_states is hidden
            if states[1] is not None:
                assert torch.equal(torch.cuda.get_rng_state(), states[1])
        learner.train(0)
        _sync(device)
        results.append((mac.actor_arena.data.clone(), mac.critic_arena.data.clone()))
    (a0, c0), (a1, c1) = results
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    return {}
