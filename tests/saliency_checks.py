"""TEST INFRASTRUCTURE: policy saliency (csrc/policy_saliency.hip, ops.saliency, DcntrlMAC.saliency) on whatever library is active -- the
host emulator in tests/test_emu_saliency.py, the gfx950 build in tests/test_gpu_saliency.py.

Ground truth: fp64 torch.autograd.grad of oracle.actor_logits -> log_softmax -> gather and of oracle.critic_value with respect to the
input rows (oracle.build_inputs_train, the one-hots as the trace defines them), the recorded state held constant; ReLU trunks take
the branch the kernel took (its act1 > 0 / act2 > 0) as ``relu_hint``.  Rule (as tests/kernel_checks.py applies it to
the actor / critic backward): error = max|got - ref64| / max|ref64| over the row set of one net, bound = max(1e-5, E32_FACTOR x the
same oracle run in fp32 against fp64); the same rule for gxi and gl1; y (logp, values) at 1e-5.  The checks never touch
``L.use_library_for_tests``.  Each returns the worst errors."""
import functools
import os

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from oracle import iplan_oracle as O
from tests.oracle_checks import E32_FACTOR, _grad_err, _Log, _rel
from tests.policy_trace_checks import _args, _bits, _codes, _e2e_args, _params, _sync, _worse, assert_out_refused, make_mac

TOL = 1e-5
M = 64
# (nA, E, S, N, d) + options.  rows = E x S: 1, 15, 16, 17 and 65 (five tiles: a second workgroup); N = 3 with d = 5: a history block of
# 15 < 16; N = 7: 35, a ragged third k-tile; N = 64: the limit; d = 4: the contiguous column path
KERNEL_CASES = [
    ((1, 1, 1, 1, 5), {}),
    ((1, 5, 3, 3, 5), {}),
    ((1, 16, 1, 7, 5), {}),
    ((1, 17, 1, 3, 4), {}),
    ((1, 13, 5, 3, 5), {}),
    ((1, 2, 2, 55, 5), {}),
    ((1, 1, 2, 64, 5), {}),
    ((1, 3, 2, 7, 4), dict(avail_ones=True)),
    ((1, 2, 2, 3, 5), dict(gat=False)),
    ((1, 2, 2, 7, 5), dict(beh=False)),
    ((1, 2, 2, 3, 5), dict(gat=False, beh=False)),
    ((1, 2, 2, 3, 5), dict(last_action=False)),
    ((2, 2, 2, 3, 5), dict(agent_id=False)),
    ((5, 2, 3, 3, 5), {}),
    ((2, 2, 2, 3, 5), dict(tanh=True)),
    ((1, 3, 2, 7, 4), dict(tanh=True, gat=False)),
    ((1, 5, 3, 3, 5), dict(which="actor", target="greedy")),
    ((1, 5, 3, 3, 5), dict(which="critic")),
    ((2, 3, 3, 3, 5), dict(steps=(1, 3))),
    ((1, 17, 1, 64, 4), dict(avail_ones=True)),
]
CASE_IDS = ["one_row_one_entity", "rows15_hist15", "rows16_ragged_ktile", "rows17_d4", "rows65_two_workgroups", "N55", "N64", "d4_avail_ones",
            "no_gat", "no_beh", "history_only", "no_last_action", "no_agent_id", "five_agents", "tanh", "tanh_d4_no_gat", "actor_only_greedy",
            "critic_only", "later_steps", "N64_d4_two_tiles"]
RUN_OPTS = ("which", "target", "steps", "avail_ones")


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


class Case:
    """a DcntrlMAC with spread-out parameters and an episode batch [E, S + 1, nA, ...] (one physical step more than is inspected, so
    T_phys > T): dense random features, avail with random zeros -- the recorded action always available, never all-zero, and in
    environment 0 both neighbours of the recorded action masked"""

    def __init__(self, dims, device, seed=0, avail_ones=False, **opt):
        from iplan_amd import synth
        nA, E, S, N, d = dims
        self.dims, self.device = dims, device
        self.args = _args(device, nA, N, d, 5, S, **opt)
        a = self.args
        self.mac = make_mac(a, 31 + seed)
        f = synth.make_episode_fields(a, E, seed=7 + seed + sum(dims), terminated_p=0.2)
        gen = torch.Generator().manual_seed(200 + seed + sum(dims))
        # input scale: LayerNorm(F) makes the nets blind to it, but d x^ / d x is orthogonal to x^ only up to the factor eps / (var + eps)
        # (eps = 1e-5 under the root): sum_k g_k x^_k = sum(g^ x^) eps / sigma^3 exactly, in any arithmetic.  With var(x) of a few units
        # that term stays below the F 2^-23 sum |g| of the invariant for every F of the cases (the fp64 figure is logged beside the kernel's)
        f["history"] = torch.rand(f["history"].shape, generator=gen) * 8 - 4
        f["attention_latent"] = torch.randn(f["attention_latent"].shape, generator=gen) * 2
        n_act = a.n_actions
        if avail_ones:
            f["avail_actions"] = torch.ones_like(f["avail_actions"])
        else:
            av = (torch.rand(f["avail_actions"].shape, generator=gen) < 0.6).int()
            rec = f["actions"][0, ..., 0]                                    # [T1, nA]
            for off in (-1, 1):
                av[0].scatter_(-1, ((rec + off) % n_act).unsqueeze(-1), 0)
            av.scatter_(-1, f["actions"], 1)
            f["avail_actions"] = av
        self.f = f
        self.T1 = S + 1
        self.batch = synth.DictBatch(f, E, self.T1).to(device)
        self.np_batch = synth.DictBatch({k: v.numpy() for k, v in f.items()}, E, self.T1)

    def run(self, which="both", target="recorded", steps=None, want=("entity", "input_grad", "act"), hidden=None, batch=None):
        S = self.dims[2]
        res = self.mac.saliency(self.batch if batch is None else batch, target=target, which=which, hidden=hidden, want=want,
                                steps=slice(0, S) if steps is None else steps)
        _sync(self.device)
        return res


@functools.lru_cache(maxsize=None)
def get_case(dims, device, opt=(), seed=0):
    return Case(dims, device, seed=seed, **dict(opt))


def build_rows(case, i, dtype, sl):
    """agent i's input rows x [E, S', F] in ``dtype`` as the kernel assembles them, and its state / avail / recorded actions"""
    a, f = case.args, case.f
    nA = a.n_agents
    hist = f["history"][:, :, i].to(dtype)
    E, T1 = hist.shape[:2]
    n_act = a.n_actions
    x = O.build_inputs_train(i, hist, f["attention_latent"][:, :, i].to(dtype), f["behavior_latent"][:, :, i].to(dtype),
                             torch.zeros(E, T1, n_act, dtype=dtype), nA, a.GAT_enable, a.Behavior_enable)
    parts = [x[..., :x.shape[-1] - n_act - nA]]
    acts = f["actions"][:, :, i, 0]
    if a.obs_last_action:
        last = torch.cat([torch.full_like(acts[:, :1], -1), acts[:, :-1]], 1)
        oh = torch.zeros(E, T1, n_act, dtype=dtype)
        oh.scatter_(-1, last.clamp_min(0).unsqueeze(-1), (last >= 0).to(dtype).unsqueeze(-1))
        parts.append(oh)
    if a.obs_agent_id:
        idoh = torch.zeros(E, T1, nA, dtype=dtype)
        idoh[..., i] = 1
        parts.append(idoh)
    return torch.cat(parts, -1)[:, sl]


def reference(case, i, dtype, sl, target, hints, hidden=None):
    """(logp [R], values [R], d logp / d x [R, F], d V / d x [R, F], x [R, F]) of agent i over the rows of steps ``sl`` in ``dtype``;
    target [E, S'] int64; hints: ((act1 > 0, act2 > 0) of the actor, ... of the critic) or None"""
    f, a = case.f, case.args
    ap, cp = _params(case.mac, dtype)
    x = build_rows(case, i, dtype, sl).flatten(0, 1).clone().requires_grad_(True)
    R = x.shape[0]
    ha = (f["rnn_states_actors"][:, sl, i] if hidden is None else hidden[0][:, :, i]).reshape(R, M).to(dtype)
    hc = (f["rnn_states_critics"][:, sl, i] if hidden is None else hidden[1][:, :, i]).reshape(R, M).to(dtype)
    av = f["avail_actions"][:, sl, i].reshape(R, -1)
    logits, _ = O.actor_logits(ap[i], x, ha, av, relu_hint=None if hints is None else hints[0], use_relu=a.use_ReLU)
    lp = torch.log_softmax(logits, -1).gather(-1, target.reshape(R, 1))[:, 0]
    ga, = torch.autograd.grad(lp.sum(), x)
    v, _ = O.critic_value(cp[i], x, hc, relu_hint=None if hints is None else hints[1], use_relu=a.use_ReLU)
    gc, = torch.autograd.grad(v[:, 0].sum(), x)
    return lp.detach(), v[:, 0].detach(), ga, gc, x.detach()


def entity_sums(case, g, x):
    """[R, F] gradient and input -> (gxi, gl1) [R, N, n_src]"""
    a = case.args
    N = a.max_vehicle_num
    widths = [w for _, w in case.mac._widths()]
    W = sum(widths)
    R = g.shape[0]
    gx = (g * x)[:, :N * W].reshape(R, N, W)
    ga = g.abs()[:, :N * W].reshape(R, N, W)
    cuts = np.cumsum([0] + widths)
    return (torch.stack([gx[..., lo:hi].sum(-1) for lo, hi in zip(cuts[:-1], cuts[1:])], -1),
            torch.stack([ga[..., lo:hi].sum(-1) for lo, hi in zip(cuts[:-1], cuts[1:])], -1))


def assert_vs_fp64(case, got, sl, worst, what, nets=("actor", "critic"), hidden=None):
    """input_grad, gxi, gl1 and y of every agent against fp64 under the rule, and the LayerNorm(F) invariant per row"""
    a = case.args
    nA = a.n_agents
    relu = a.use_ReLU
    for i in range(nA):
        tgt = got["target_action"][:, :, i].cpu() if "target_action" in got else case.f["actions"][:, sl, i, 0]
        hints = None
        if relu:
            hints = tuple((got[n + "_act1"][:, :, i].cpu().flatten(0, 1) > 0, got[n + "_act2"][:, :, i].cpu().flatten(0, 1) > 0) if n in nets else None
                          for n in ("actor", "critic"))
            hints = tuple(h if h is not None else hints[1 - k] for k, h in enumerate(hints))
        r64 = reference(case, i, torch.float64, sl, tgt, hints, hidden)
        r32 = reference(case, i, torch.float32, sl, tgt, hints, hidden)
        x64 = r64[4]
        F = x64.shape[1]
        xh = (x64 - x64.mean(-1, keepdim=True)) / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-5)
        for k, net in enumerate(("actor", "critic")):
            if net not in nets:
                continue
            ykey = "logp" if net == "actor" else "values"
            ey = _rel(got[ykey][:, :, i].cpu().flatten(), r64[k])
            print(what, net, i, ykey, "err", ey)
            _worse(worst, ykey, ey)
            assert ey <= TOL, (what, net, i, ykey, ey)
            g = got[net + "_input_grad"][:, :, i].cpu().flatten(0, 1)
            refs = dict(input_grad=(g, r64[2 + k], r32[2 + k]))
            e64, e32_ = entity_sums(case, r64[2 + k], x64), entity_sums(case, r32[2 + k], r32[4])
            refs["gxi"] = (got[net + "_gxi"][:, :, i].cpu().flatten(0, 1), e64[0], e32_[0])
            refs["gl1"] = (got[net + "_gl1"][:, :, i].cpu().flatten(0, 1), e64[1], e32_[1])
            for key, (gv, ref, ref32) in refs.items():
                assert gv.shape == ref.shape, (key, gv.shape, ref.shape)
                assert ref.abs().max() > 0, (what, net, key, "the reference gradient is zero: the case checks nothing")
                err, e32 = _grad_err(gv, ref), _grad_err(ref32, ref)
                print(what, net, i, key, "err", err, "e32", e32)
                _worse(worst, net + "_" + key, err)
                _worse(worst, net + "_" + key + "_e32", e32)
                assert err <= _bound(e32), (what, net, i, key, err, e32)
            # the gradient of a normalised input is orthogonal to 1 and to x^
            gd = g.double()
            l1 = gd.abs().sum(-1)
            lim = F * 2.0 ** -23 * l1
            s_one, s_xh = gd.sum(-1).abs(), (gd * xh).sum(-1).abs()
            g64 = r64[2 + k]
            lim64 = F * 2.0 ** -23 * g64.abs().sum(-1)
            _worse(worst, net + "_ln_xhat_over_bound_fp64_oracle", ((g64 * xh).sum(-1).abs() / lim64.clamp_min(1e-300)).max())
            print(what, net, i, "LN(F) invariant / bound: sum", (s_one / lim).max().item(), "x^", (s_xh / lim).max().item(), "x^ of the fp64 oracle",
                  worst[net + "_ln_xhat_over_bound_fp64_oracle"])
            _worse(worst, net + "_ln_sum_over_bound", (s_one / lim.clamp_min(1e-300)).max())
            _worse(worst, net + "_ln_xhat_over_bound", (s_xh / lim.clamp_min(1e-300)).max())
            assert (s_one <= lim).all(), (what, net, i, "sum of the input gradient", (s_one / lim).max().item())
            assert (s_xh <= lim).all(), (what, net, i, "input gradient . x^", (s_xh / lim).max().item())


# ------------------------------------------------------------------------------------------------ the kernel against fp64
def check_kernel(device, dims, opt):
    """1: input_grad, the entity sums and y of every net and agent against fp64; the LayerNorm(F) invariant; shapes and sources"""
    run = {k: v for k, v in opt.items() if k in RUN_OPTS}
    case = get_case(dims, device, tuple(sorted((k, v) for k, v in opt.items() if k not in RUN_OPTS or k == "avail_ones")))
    nA, E, S, N, d = dims
    which = run.get("which", "both")
    steps = slice(*run["steps"]) if "steps" in run else slice(0, S)
    got = case.run(which=which, target=run.get("target", "recorded"), steps=steps)
    nets = ("actor", "critic") if which == "both" else (which,)
    Sn = steps.stop - steps.start
    n_src = len(case.mac._widths())
    assert got["sources"] == tuple(k for k, _ in case.mac._widths())
    for net in ("actor", "critic"):
        for key, shape in (("gxi", (E, Sn, nA, N, n_src)), ("gl1", (E, Sn, nA, N, n_src)), ("input_grad", (E, Sn, nA, case.mac.input_shape))):
            assert (net + "_" + key in got) == (net in nets), (net, key)
            if net in nets:
                assert got[net + "_" + key].shape == shape and got[net + "_" + key].dtype == torch.float32, (net, key, got[net + "_" + key].shape)
    assert ("values" in got) == ("critic" in nets) and ("logp" in got) == ("target_action" in got) == ("actor" in nets)
    if "actor" in nets:
        assert got["target_action"].dtype == torch.int64
        if run.get("target", "recorded") == "recorded":
            assert torch.equal(got["target_action"].cpu(), case.f["actions"][:, steps, :, 0])
    worst = {}
    assert_vs_fp64(case, got, steps, worst, (dims, opt), nets)
    return worst


def check_greedy_matches_trace(device, dims=(2, 3, 3, 3, 5)):
    """2: the greedy target equals policy_trace's greedy on the same rows and states; logp (of the recorded action) and values agree
    with policy_trace within 1e-5"""
    case = get_case(dims, device)
    nA, E, S = dims[:3]
    worst = {}
    gr = case.run(target="greedy", want=())
    rec = case.run(want=())
    for s in range(S):                                                       # one-step traces from the recorded states: the same rows
        res, _, _ = case.mac._trace(case.batch, s, 1, None, "both", ("greedy", "logp", "values"), False)
        _sync(device)
        assert torch.equal(gr["target_action"][:, s], res["greedy"][:, :, 0].t()), ("greedy", s)
        for key, mine in (("logp", rec["logp"]), ("values", rec["values"])):
            diff = (mine[:, s] - res[key][:, :, 0].t()).abs().max().item()
            print("saliency vs policy_trace", key, "step", s, "diff", diff)
            _worse(worst, key + "_vs_trace", diff)
            assert diff <= TOL, (key, s, diff)
        assert torch.equal(gr["values"][:, s], rec["values"][:, s])
    return worst


def _same(a, b, what):
    for k in sorted(set(a) & set(b)):
        if k != "sources":
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, "bits differ")


def check_placement(device, reps=2):
    """3: two calls give the same bits; a row gives the same bits as the only row, as row 16 of 17 and under a steps= restriction;
    packed and in-place fc1 operands give the same bits"""
    from iplan_amd import synth
    dims = (1, 17, 1, 3, 5)
    case = get_case(dims, device)
    full = case.run()
    for _ in range(reps - 1):
        _same(case.run(), full, "repeat")
    for e in (0, 16):                                                        # row e of 17 alone: lane 0 of the only tile
        one = synth.DictBatch({k: v[e:e + 1].clone() for k, v in case.f.items()}, 1, case.T1).to(device)
        alone = case.run(batch=one)
        _same(alone, {k: (v if k == "sources" else v[e:e + 1]) for k, v in full.items()}, ("alone", e))
    multi = get_case((2, 3, 3, 3, 5), device)
    whole = multi.run()
    for s0, s1 in ((0, 1), (1, 3), (2, 3)):
        part = multi.run(steps=slice(s0, s1))
        _same(part, {k: (v if k == "sources" else v[:, s0:s1]) for k, v in whole.items()}, ("steps", s0, s1))
    single = multi.run(steps=1)
    _same(single, {k: (v if k == "sources" else v[:, 1]) for k, v in whole.items()}, "steps=int")
    assert multi.mac.fc1_pack.get is not None
    keep = os.environ.get("IPLAN_NO_FC1_PACK")
    os.environ["IPLAN_NO_FC1_PACK"] = "1"                                    # Fc1Pack.get returns None: the arena is read in place
    try:
        assert multi.mac.fc1_pack.get(None) is None
        inplace = multi.run()
    finally:
        if keep is None:
            del os.environ["IPLAN_NO_FC1_PACK"]
        else:
            os.environ["IPLAN_NO_FC1_PACK"] = keep
    _same(inplace, whole, "packed != in place")
    return {}


class _Injected:
    """ops.saliency / ops.saliency_args seen through the method: ``out`` is handed to the launch, the descriptor is recorded"""

    def __init__(self, out=None, launch=True):
        self.out, self.launch, self.seen = out, launch, None

    def __enter__(self):
        self.orig = ops.saliency_args
        inj = self

        def wrapped(*a, **kw):
            a = list(a)
            if len(a) >= 19:
                a[18] = inj.out if inj.out is not None else a[18]
            else:
                kw["out"] = inj.out if inj.out is not None else kw.get("out")
            inj.seen = inj.orig(*a, **kw)
            return inj.seen
        ops.saliency_args = wrapped
        return self

    def __exit__(self, *exc):
        ops.saliency_args = self.orig


OUT_KEYS = ("logp", "values", "target_action", "entity_actor", "entity_critic", "input_grad_actor", "input_grad_critic", "act1_actor", "act2_actor",
            "act1_critic", "act2_critic")


def _sentinels(shapes, device, shift=0.0):
    bufs = {}
    for k, shape in shapes.items():
        n = int(np.prod(shape))
        if k == "target_action":
            sent = torch.arange(n + 64, dtype=torch.int64) * 7 + 1000
        else:
            sent = 0.5 + shift + (torch.arange(n + 64, dtype=torch.float32) % 1021) / 1024.0
        buf = sent.clone().to(device)
        bufs[k] = (sent, buf, buf[32:32 + n].view(shape))
    return bufs


def _out_shapes(case, Sn):
    nA, E, S, N, d = case.dims
    F, n_src = case.mac.input_shape, len(case.mac._widths())
    sh = dict(logp=(nA, E, Sn), values=(nA, E, Sn), target_action=(nA, E, Sn))
    for net in ("actor", "critic"):
        sh["entity_" + net] = (nA, E, Sn, N, n_src, 2)
        sh["input_grad_" + net] = (nA, E, Sn, F)
        sh["act1_" + net] = sh["act2_" + net] = (nA, E, Sn, M)
    return sh


def check_sentinel(device):
    """4: outputs carved out of sentinel-filled buffers at three ragged shapes: nothing outside the owned region is written, every owned
    element is, and an output that was not asked for stays untouched"""
    for dims, opt in (((2, 3, 3, 3, 5), {}), ((1, 17, 1, 7, 5), {}), ((1, 5, 1, 3, 4), dict(gat=False))):
        case = get_case(dims, device, tuple(sorted(opt.items())))
        S = dims[2]
        shapes = _out_shapes(case, S)
        with _Injected() as inj:
            case.run()
            ref = dict(inj.seen[1])
        assert set(ref) == set(OUT_KEYS)
        for which, want in (("both", ("entity", "input_grad", "act")), ("both", ("entity",)), ("actor", ("input_grad",)), ("critic", ())):
            bufs = _sentinels(shapes, device)
            with _Injected(out={k: v[2] for k, v in bufs.items()}) as inj:
                case.run(which=which, want=want)
                got = dict(inj.seen[1])
            nets = ("actor", "critic") if which == "both" else (which,)
            owned = {k for k in OUT_KEYS if (k in ("logp", "target_action") and "actor" in nets) or (k == "values" and "critic" in nets)
                     or any(k == w + "_" + n or (w == "act" and k in ("act1_" + n, "act2_" + n)) for w in want for n in nets)}
            assert set(got) == owned, (which, want, sorted(got), sorted(owned))
            for k, (sent, buf, view) in bufs.items():
                host = buf.cpu()
                if k not in owned:
                    assert torch.equal(host, sent), (dims, which, want, k, "was not asked for and was written")
                    continue
                assert torch.equal(_bits(view), _bits(ref[k])), (dims, k, "differs inside a padded buffer")
                n = view.numel()
                assert torch.equal(host[:32], sent[:32]) and torch.equal(host[32 + n:], sent[32 + n:]), (dims, k, "an element outside the owned region was written")
        b2 = _sentinels(shapes, device, 0.25)                 # every owned element is written: a second, shifted sentinel ends the same
        with _Injected(out={k: v[2] for k, v in b2.items()}):
            case.run()
        for k in OUT_KEYS:
            assert torch.equal(_bits(b2[k][2]), _bits(ref[k])), (dims, k, "an owned element was left unwritten")
    return {}


def _learner(device, seed=6):
    from iplan_amd import synth
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    from iplan_amd.learners.ippo_learner import IPPOLearner
    from tests.oracle_checks import _fields
    args = _e2e_args(device, episode_limit=9)
    torch.manual_seed(seed)
    scheme = synth.make_scheme(args)
    mac = DcntrlMAC(scheme, {"agents": args.n_agents}, args)
    learner = IPPOLearner(mac, scheme, _Log(), args)
    E = args.buffer_size
    _, batch = _fields(args, E, 7, 0.15, device)
    learner.batch_size_run = E
    learner.insert_episode_batch(batch)
    return args, mac, learner, batch


def _state_tensors(obj, seen=None, depth=0):
    """every tensor reachable from an optimiser-like object's attributes (Adam moments, step counters, ...)"""
    out = []
    seen = set() if seen is None else seen
    if id(obj) in seen or depth > 4:
        return out
    seen.add(id(obj))
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, dict):
        for v in obj.values():
            out += _state_tensors(v, seen, depth + 1)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            out += _state_tensors(v, seen, depth + 1)
    elif hasattr(obj, "__dict__") and type(obj).__module__.startswith("iplan_amd"):
        for v in vars(obj).values():
            out += _state_tensors(v, seen, depth + 1)
    return out


def check_touches_nothing(device):
    """5: parameters, both arenas' gradient entries (pre-filled with a sentinel), the optimisers' state, hidden_states, the batch and
    the torch generator states are bit-identical before and after saliency(); a train() after saliency() gives the bits of one
    without it"""
    results = []
    for with_saliency in (False, True):
        args, mac, learner, batch = _learner(device)
        torch.manual_seed(83)
        if with_saliency:
            for arena in (mac.actor_arena, mac.critic_arena):
                arena.grad.fill_(0.7071)
            watched = [t for t in _state_tensors(learner) if t.device.type == torch.device(device).type]
            assert any(t.data_ptr() == mac.actor_arena.data.data_ptr() for t in watched) and len(watched) > 8, len(watched)
            before = [t.clone() for t in watched]
            fields = {k: v.clone() for k, v in batch.data.items()}
            states = (torch.get_rng_state(), torch.cuda.get_rng_state() if torch.device(device).type == "cuda" else None)
            mac.hidden_states = "untouched"
            res = mac.saliency(batch, want=("entity", "input_grad"))
            _sync(device)
            assert torch.isfinite(res["actor_gxi"]).all() and torch.isfinite(res["critic_input_grad"]).all() and res["actor_gl1"].abs().sum() > 0
            assert torch.equal(torch.get_rng_state(), states[0])
            if states[1] is not None:
                assert torch.equal(torch.cuda.get_rng_state(), states[1])
            assert mac.hidden_states == "untouched"
            mac.hidden_states = None
            for t, b in zip(watched, before):
                assert torch.equal(_bits(t), _bits(b)), ("a tensor of the learner changed", tuple(t.shape))
            for arena in (mac.actor_arena, mac.critic_arena):
                assert torch.equal(arena.grad, torch.full_like(arena.grad, 0.7071)), "a gradient entry was written"
                arena.grad.zero_()
            for k, v in fields.items():
                assert torch.equal(batch.data[k], v), (k, "the batch was written")
        else:
            for arena in (mac.actor_arena, mac.critic_arena):
                arena.grad.zero_()
        learner.train(0)
        _sync(device)
        results.append((mac.actor_arena.data.clone(), mac.critic_arena.data.clone()))
    (a0, c0), (a1, c1) = results
    assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    return {}


def check_host_api(device, dims=(2, 3, 3, 3, 5)):
    """6: numpy in -> numpy out; a device EpisodeBatch-like batch with steps=int; hidden= given tensors; target= tensor -- all agree"""
    case = get_case(dims, device)
    nA, E, S = dims[:3]
    worst = {}
    dev = case.run()
    as_np = case.run(batch=case.np_batch)
    for k, v in dev.items():
        if k == "sources":
            assert as_np[k] == v
            continue
        assert isinstance(as_np[k], np.ndarray) and torch.is_tensor(v) and v.device.type == torch.device(device).type, k
        assert np.array_equal(as_np[k], v.cpu().numpy()), (k, "numpy-backed and device-backed batches differ")
    for t in (0, 2):
        one = case.run(steps=t)
        for k, v in one.items():
            if k != "sources":
                assert v.shape == dev[k].shape[:1] + dev[k].shape[2:] and torch.equal(_bits(v), _bits(dev[k][:, t])), (k, t)
    hid = (case.f["rnn_states_actors"][:, :S].clone(), case.f["rnn_states_critics"][:, :S].numpy().copy())
    _same(case.run(hidden=hid), dev, "hidden= the recorded states")
    gen = torch.Generator().manual_seed(5)
    other = (torch.randn(E, S, nA, M, generator=gen) * 0.3, torch.randn(E, S, nA, M, generator=gen) * 0.3)
    got = case.run(hidden=other)
    assert not torch.equal(got["values"], dev["values"])
    assert_vs_fp64(case, got, slice(0, S), worst, "hidden= given", hidden=other)
    _same(case.run(target=case.f["actions"][:, :S, :, 0]), dev, "target= the recorded actions")
    _same(case.run(target=torch.full((E, S, nA), -1).numpy()), case.run(target="greedy"), "target= -1")
    tgt = torch.randint(0, case.args.n_actions, (E, S, nA), generator=gen)
    tgt = torch.where(case.f["avail_actions"][:, :S].gather(-1, tgt.unsqueeze(-1))[..., 0] > 0, tgt, case.f["actions"][:, :S, :, 0])
    got = case.run(target=tgt.to(device))
    assert torch.equal(got["target_action"].cpu(), tgt)
    assert_vs_fp64(case, got, slice(0, S), worst, "target= tensor")
    return worst


def check_bad_arguments(device, dims=(2, 3, 3, 3, 5)):
    """7: each invalid descriptor is refused by the host-side check with a negative IPLAN_E* code and a message; an ``out=`` destination
    of the wrong shape or dtype, or a non-contiguous one, makes ops.saliency raise AssertionError; nothing is launched, so the
    sentinel-filled outputs stay as they were.  saliency() refuses layer_N = 2"""
    case = get_case(dims, device)
    S = dims[2]
    good = case.run()
    bufs = _sentinels(_out_shapes(case, S), device)
    with _Injected(out={k: v[2] for k, v in bufs.items()}) as inj:
        case.run()
        a, res, keep = inj.seen
    fresh = _sentinels(_out_shapes(case, S), device)
    for k, v in fresh.items():                                               # back to sentinels: only the refused calls follow
        bufs[k][1].copy_(v[1])
    _sync(device)
    lib = ops._lib(None)
    EINVAL = _codes()
    fn = lib.c.iplan_ac_saliency

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
        assert rc == EINVAL and rc < 0 and "iplan_ac_saliency" in msg, (fields, rc, msg)

    refused(None)
    ref = L.C.byref(a)
    refused(ref, **{"feat.N": 65})
    refused(ref, **{"feat.N": 0})
    refused(ref, **{"feat.N": -3})
    refused(ref, E=0)
    refused(ref, S=0)
    refused(ref, E=-1)
    refused(ref, h_actor=None)
    refused(ref, h_critic=None)
    refused(ref, target=None, target_all=-2)
    refused(ref, target=None, target_all=case.args.n_actions)
    refused(ref, which=3)
    none = {k: None for k in ("logp", "values", "target_out", "entity_actor", "entity_critic", "input_grad_actor", "input_grad_critic", "act1_actor",
                              "act2_actor", "act1_critic", "act2_critic")}
    refused(ref, **none)
    refused(ref, which=1, **{k: None for k in none if k.endswith("critic") or k == "values"})          # only actor outputs, critics asked for

    def with_out(out):                                                       # ops.saliency, called by the method with this ``out``
        with _Injected(out=out):
            case.run()
    assert_out_refused(with_out, bufs, ("logp", "target_action", "entity_critic"))
    _sync(device)
    for k, (sent, buf, _) in bufs.items():
        assert torch.equal(buf.cpu(), sent), (k, "a refused call wrote an output")
    _same(case.run(), good, "after the refusals")
    del keep, res
    # layer_N = 2: R_Actor's constructor already refuses it, so no DcntrlMAC exists in that configuration; the method is asked on an
    # instance whose args are set afterwards, where it refuses as _trace does
    import copy
    mac = case.mac
    orig = mac.args
    try:
        mac.args = copy.copy(orig)
        mac.args.layer_N = 2
        for call in (lambda: mac.saliency(case.batch), lambda: mac._trace(case.batch, 0, 1, None, "both", ("values",), False)):
            try:
                call()
            except NotImplementedError:
                pass
            else:
                raise AssertionError("layer_N = 2 was not refused")
        mac.args.layer_N, mac.args.recurrent_N = 1, 2
        try:
            mac.saliency(case.batch)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("recurrent_N = 2 was not refused")
    finally:
        mac.args = orig
    return {}
