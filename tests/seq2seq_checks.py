"""TEST INFRASTRUCTURE: the two Seq2Seq kernels alone (csrc/seq2seq.hip: iplan_seq2seq_fwd in its saving and non-saving form,
iplan_seq2seq_bwd), on whatever library is active -- the host emulator in tests/test_emu_seq2seq.py, the gfx950 build in
tests/test_gpu_seq2seq.py.  The descriptors are filled directly and launched with ``lib.call``; the parameter block and its offsets
come from a ParamArena over a Seq2Seq module, as Seq2Seq.forward takes them; the parameter gradients are
iplan_amd.nova.Seq2Seq.seq2seq_backward on the same record.

Ground truth: the unchanged oracle.seq2seq_forward in fp64 with fp64 autograd under the linear loss sum(out * gw); for the record
(``save``) and the row gradients (``dsave``) the step-by-step reference below (_stepwise), which keeps the gates and whose output is
held to the oracle's to 1e-13.  Both run in fp32 beside it.  Rule: bound = max(1e-5, E32_FACTOR x e32), e32 the
fp32 reference's error by the same measure; out, hidden_out and every field of the record on the scale max(1, max|ref|); every
parameter gradient on its own scale per tensor (oracle_checks._grad_err); every field of dsave on its own scale per field, layer
and stack.  A cell that is exactly zero in fp64 must be exactly zero: the columns >= O of the decoder-input block and of the d out
block, the first encoder step's h_prev, every row gradient of a row whose dropout flags are all 0.

Every launch (launch()) puts each output FENCE floats inside a sentinel-filled buffer, pre-filled with NaN, and holds: the fences
intact, no NaN left inside, every input and the parameter block bit-unchanged.  ``shift`` moves every tensor base that many floats
off its 16-byte alignment; ``pad`` is what lies behind the last row of every input (and in the teacher cells the contract does not
read).  The checks never touch ``L.use_library_for_tests``; each returns the worst errors it measured."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import torch

from iplan_amd import _lib as L
from iplan_amd.nova.gat_function import _GradSink
from iplan_amd.nova.Seq2Seq import Seq2Seq, save_floats, seq2seq_backward
from oracle import iplan_oracle as O
from tests.ac_backward_checks import _sentinel
from tests.oracle_checks import E32_FACTOR, _grad_err
from tests.ppo_eval_checks import _bits, _einval, _sync, _worse

TOL = 1e-5
FENCE = 64
DROP_P = 0.25
NAN = float("nan")

# feedback: "none" = no teacher; otherwise the coins of a teacher: "zeros", "ones", "first", "last", "alt" (0 1 0 1 ..: step 1 is fed
# step 0's prediction, step 2 the teacher's location).  dropout: "keep" = flags given with drop_p = 0.25, "none" = keep NULL.
Case = namedtuple("Case", "In H layers P O rows T_in feedback dropout", defaults=("alt", "keep"))


def _c(In=5, H=32, layers=2, P=3, O=2, rows=65, T_in=2, **kw):
    return Case(In, H, layers, P, O, rows, T_in, **kw)


ROWS = (1, 15, 16, 17, 63, 64, 65, 129)                            # 129: three workgroups, the last with one row
ROW_CASES = [_c(rows=r) for r in ROWS] + [_c(H=64, layers=4, rows=r) for r in ROWS]    # 4 x 64: the 64 KiB carry of the backward
IN_CASES = [_c(In=i) for i in (1, 3, 15, 16, 17, 33, 47, 48, 49, 63, 64)]
O_CASES = [_c(O=o) for o in (1, 2, 3, 4, 5, 15, 16)]
STACK_CASES = [_c(H=h, layers=n, rows=17) for h in (32, 64) for n in (1, 2, 3, 4)]
STEP_CASES = [_c(T_in=1), _c(P=1), _c(T_in=1, P=1, rows=17), _c(T_in=1, P=24, rows=17)]
FEEDBACK = ("none", "zeros", "ones", "first", "last")
FEEDBACK_CASES = [_c(P=4, feedback=f) for f in FEEDBACK]
DROPOUT_CASES = [_c(dropout="none"), _c(dropout="none", feedback="none"), _c(H=64, layers=1, In=17, O=5, dropout="keep")]
LARGEST = _c(In=17, H=64, layers=4, P=3, O=5, rows=129, T_in=2)
ALONE = (0, 15, 16, 63, 64, 127, 128)                              # rows launched alone: a first and a last lane of a wave, per workgroup


def case_id(c):
    return f"In{c.In}_H{c.H}_L{c.layers}_P{c.P}_O{c.O}_rows{c.rows}_T{c.T_in}_{c.feedback}_{c.dropout}"


def _bound(e32):
    return max(TOL, E32_FACTOR * e32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu())), (what, "bits differ")


def coins_of(c):
    if c.feedback == "none":
        return None
    return {"zeros": [0] * c.P, "ones": [1] * c.P, "first": [1] + [0] * (c.P - 1), "last": [0] * (c.P - 1) + [1],
            "alt": [t % 2 for t in range(c.P)]}[c.feedback]


# ================================================================================================ inputs and references
@functools.lru_cache(maxsize=None)
def make_params(In, H, layers, P, O):
    """the state_dict of a freshly initialised Seq2Seq (nn.GRU / nn.Linear defaults), fp32 on the host, never modified"""
    with torch.random.fork_rng():
        torch.manual_seed(7000 + In + 67 * H + 5 * layers + 1009 * O)
        net = Seq2Seq(In, H, layers, P, num_node=1, output_size=O, dropout=DROP_P)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


_nets = {}


def net_on(device, c):
    """-> (module, its ParamArena on ``device``), one per shape and device"""
    key = (str(device), c.In, c.H, c.layers, c.O)
    if key not in _nets:
        net = Seq2Seq(c.In, c.H, c.layers, c.P, num_node=1, output_size=c.O, dropout=DROP_P)
        net.load_state_dict(make_params(c.In, c.H, c.layers, c.P, c.O))
        _nets[key] = (net, net._own_arena(device))
    return _nets[key]


@functools.lru_cache(maxsize=None)
def make_data(c):
    """fp32 host tensors, never modified: x [R, T, In], last [R, O], teacher / gw [R, P, O], keep [P, R, H] (row 0 every flag 0, the
    last row every flag 1 where there are two rows)"""
    gen = torch.Generator().manual_seed(31 * c.In + 7 * c.H + 3 * c.layers + 101 * c.P + 1013 * c.O + 13 * c.rows + 17 * c.T_in)
    u = lambda *s: torch.rand(*s, generator=gen) * 2 - 1  # noqa: E731
    d = dict(x=u(c.rows, c.T_in, c.In), last=u(c.rows, c.O), teacher=u(c.rows, c.P, c.O), gw=u(c.rows, c.P, c.O),
             keep=(torch.rand(c.P, c.rows, c.H, generator=gen) > DROP_P).float())
    if c.rows > 1:
        d["keep"][:, 0] = 0.0
        d["keep"][:, c.rows - 1] = 1.0
    return d


def take(d, idx):
    """the rows ``idx`` of a data dict"""
    idx = torch.as_tensor(idx)
    return {k: (v[:, idx] if k == "keep" else v[idx]).contiguous() for k, v in d.items()}


def _stepwise(p, x, last, P, teacher, coins, keep, drop_p):
    """oracle.seq2seq_forward step by step, keeping what the kernels record -> out [R, P, O] and the list of per-GRU-step dicts
    (encoder steps first, layer inside step) and per-decoder-step dicts; the pre-activations and ``out`` retain their gradients"""
    layers = sum(1 for k in p if k.startswith("encoder.rnn.weight_ih_l"))
    H = p["encoder.rnn.weight_hh_l0"].shape[1]
    R = x.shape[0]
    h = [torch.zeros(R, H, dtype=x.dtype) for _ in range(layers)]
    cells, dec = [], []

    def cell(stack, k, xin, hp):
        gi = xin @ p[f"{stack}.rnn.weight_ih_l{k}"].t() + p[f"{stack}.rnn.bias_ih_l{k}"]
        gh = hp @ p[f"{stack}.rnn.weight_hh_l{k}"].t() + p[f"{stack}.rnn.bias_hh_l{k}"]
        a_r, a_z, gi_n, gh_n = gi[..., :H] + gh[..., :H], gi[..., H:2 * H] + gh[..., H:2 * H], gi[..., 2 * H:], gh[..., 2 * H:]
        for t in (a_r, a_z, gi_n, gh_n):
            t.retain_grad()
        r, z = torch.sigmoid(a_r), torch.sigmoid(a_z)
        n = torch.tanh(gi_n + r * gh_n)
        hn = (1.0 - z) * n + z * hp
        cells.append(dict(h_prev=hp, r=r, z=z, n=n, gh_n=gh_n, h_new=hn, pre=(a_r, a_z, gi_n, gh_n)))
        return hn

    for t in range(x.shape[1]):
        xin = x[:, t]
        for k in range(layers):
            xin = h[k] = cell("encoder", k, xin, h[k])
    y = last
    outs = []
    for t in range(P):
        xin = y
        for k in range(layers):
            xin = h[k] = cell("decoder", k, xin, h[k])
        act = torch.tanh(xin)
        if keep is not None:
            act = act * keep[t] / (1.0 - drop_p)
        out = act @ p["decoder.linear.weight"].t() + p["decoder.linear.bias"]
        out.retain_grad()
        dec.append(dict(yin=y, act=act, out=out))
        outs.append(out)
        y = teacher[:, t] if (teacher is not None and coins is not None and coins[t]) else out
    return torch.stack(outs, dim=1), cells, dec, h


def reference_of(c, d, dt):
    """-> dict in ``dt``: out [R, P, O], hidden [layers, R, H], grads {name: tensor} (the oracle and its autograd), save
    [steps, layers, R, 6, H], dec [P, R, 16 + H], dsave [steps, layers, R, 4, H], ddec [P, R, 16] (the step-by-step reference)"""
    R, H, steps = d["x"].shape[0], c.H, c.T_in + c.P
    coins = coins_of(c)
    x, last, gw = d["x"].to(dt), d["last"].to(dt), d["gw"].to(dt)
    teacher = d["teacher"].to(dt) if coins is not None else None
    keep = d["keep"].to(dt) if c.dropout == "keep" else None
    p = {k: v.to(dt).clone().requires_grad_(True) for k, v in make_params(c.In, c.H, c.layers, c.P, c.O).items()}
    out = O.seq2seq_forward(p, x, last.unsqueeze(1), c.P, teacher, coins, keep.reshape(c.P, R, 1, H) if keep is not None else None, DROP_P)
    (out * gw).sum().backward()
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    out_s, cells, dec, h = _stepwise(q, x, last, c.P, teacher, coins, keep, DROP_P)
    if dt == torch.float64:
        assert (out_s - out).abs().max().item() <= 1e-13, "the step-by-step reference left the oracle"
    (out_s * gw).sum().backward()
    g = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    save = torch.stack([torch.stack([cl[k].detach() for k in ("h_prev", "r", "z", "n", "gh_n", "h_new")], dim=1) for cl in cells])
    dsave = torch.stack([torch.stack([g(t) for t in cl["pre"]], dim=1) for cl in cells])
    pad = lambda t: torch.cat([t, torch.zeros(R, 16 - c.O, dtype=dt)], dim=1)  # noqa: E731
    return dict(out=out.detach(), hidden=torch.stack([t.detach() for t in h]), grads={k: v.grad for k, v in p.items()},
                save=save.view(steps, c.layers, R, 6, H).contiguous(),
                dec=torch.stack([torch.cat([pad(s["yin"].detach()), s["act"].detach()], dim=1) for s in dec]),
                dsave=dsave.view(steps, c.layers, R, 4, H).contiguous(), ddec=torch.stack([pad(g(s["out"])) for s in dec]))


@functools.lru_cache(maxsize=None)
def reference(c, dt):
    """the reference of the committed case, computed once and never modified"""
    return reference_of(c, make_data(c), dt)


# ================================================================================================ launches
def _in_buf(t, device, shift, pad):
    n = t.numel()
    host = torch.full((shift + n + FENCE,), pad, dtype=torch.float32)
    host[shift:shift + n] = t.reshape(-1)
    buf = host.to(device)
    return host, buf, buf[shift:shift + n]


def _out_buf(n, device, shift):
    sent = _sentinel(n + 2 * FENCE + shift, "cpu")
    host = sent.clone()
    host[FENCE + shift:FENCE + shift + n] = NAN
    buf = host.to(device)
    return sent, buf, buf[FENCE + shift:FENCE + shift + n]


def _fence_intact(sent, buf, lo, n, what):
    host = buf.cpu()
    assert torch.equal(_bits(host[:lo]), _bits(sent[:lo])) and torch.equal(_bits(host[lo + n:]), _bits(sent[lo + n:])), (what, "written outside its extent")
    assert not torch.isnan(host[lo:lo + n]).any(), (what, "a cell inside its extent was left unwritten")


def fill_args(device, c, d, ins, shift=0):
    """IplanSeq2SeqArgs of case ``c`` over the input views ``ins`` (x, last and, where the case has them, teacher, coins, keep)"""
    net, arena = net_on(device, c)
    a = L.Seq2SeqArgs()
    a.rows, a.T_in, a.In, a.H, a.layers, a.P, a.O = d["x"].shape[0], c.T_in, c.In, c.H, c.layers, c.P, c.O
    a.x, a.last = ins["x"].data_ptr(), ins["last"].data_ptr()
    if "teacher" in ins:
        a.teacher, a.coins = ins["teacher"].data_ptr(), ins["coins"].data_ptr()
    if "keep" in ins:
        a.keep, a.drop_p = ins["keep"].data_ptr(), DROP_P
    a.params = arena.data.data_ptr()
    for k in range(c.layers):
        for j, nm in enumerate(("weight_ih", "weight_hh", "bias_ih", "bias_hh")):
            a.enc_off[4 * k + j] = arena.off(f"encoder.rnn.{nm}_l{k}")
            a.dec_off[4 * k + j] = arena.off(f"decoder.rnn.{nm}_l{k}")
    a.lin_off[0], a.lin_off[1] = arena.off("decoder.linear.weight"), arena.off("decoder.linear.bias")
    return a


def launch(device, c, d=None, shift=0, pad=0.0, saving=True, hidden=True, backward=True, grads=False, drop_p_without_keep=False):
    """the forward launch of case ``c`` on the rows ``d`` (default: the committed ones) and, with ``backward``, iplan_seq2seq_bwd on its
    record; ``grads``: the parameter gradients too (seq2seq_backward: a launch of its own and the contractions).  -> dict of device
    tensors: out [R, P, O], hidden [layers, R, H], save [steps, layers, R, 6, H], dec [P, R, 16 + H], dsave [steps, layers, R, 4, H],
    ddec [P, R, 16], grads {name: tensor}"""
    d = d or make_data(c)
    R, H, steps = d["x"].shape[0], c.H, c.T_in + c.P
    coins = coins_of(c)
    lib, stream = L.get_lib(), L.current_stream(device)
    net, arena = net_on(device, c)
    params_before = arena.data.cpu().clone()
    host_in = dict(x=d["x"], last=d["last"], gw=d["gw"])
    if coins is not None:
        tl = d["teacher"].clone()
        unread = [t for t in range(c.P) if not coins[t] or t == c.P - 1]       # (the last step's teacher cell feeds no step)
        tl[:, unread] = pad
        host_in["teacher"] = tl
    if c.dropout == "keep":
        host_in["keep"] = d["keep"]
    bufs = {k: _in_buf(v, device, shift, pad) for k, v in host_in.items()}
    ins = {k: v[2] for k, v in bufs.items()}
    if coins is not None:
        ins["coins"] = torch.tensor(coins, dtype=torch.int32).to(device)
    a = fill_args(device, c, d, ins, shift)
    if drop_p_without_keep:
        assert c.dropout == "none"
        a.drop_p = DROP_P
    n_save, n_dsave = save_floats(R, c.T_in, c.P, c.layers, H)
    sizes = dict(out=R * c.P * c.O)
    if hidden:
        sizes["hidden"] = c.layers * R * H
    if saving:
        sizes["save"] = n_save
        if backward:
            sizes["dsave"] = n_dsave
    outs = {k: _out_buf(n, device, shift) for k, n in sizes.items()}
    a.out = outs["out"][2].data_ptr()
    a.hidden_out = outs["hidden"][2].data_ptr() if hidden else None
    a.save = outs["save"][2].data_ptr() if saving else None
    lib.call("iplan_seq2seq_fwd", a, stream)
    got = {}
    if saving and backward:
        b = L.Seq2SeqBwdArgs()
        b.fwd = a
        b.g_out, b.dsave = ins["gw"].data_ptr(), outs["dsave"][2].data_ptr()
        lib.call("iplan_seq2seq_bwd", b, stream)
    if grads:
        assert saving and shift == 0
        sink = _GradSink(arena)
        seq2seq_backward(sink, a, outs["save"][2], ins["gw"].view(R, c.P, c.O))
        got["grads"] = {k: sink.grad[0, arena.offsets[k]:arena.offsets[k] + int(np.prod(arena.shapes[k]))].view(arena.shapes[k]).clone() for k in arena.names}
    _sync(device)
    what = (case_id(c), R, "shift", shift)
    for k, (sent, buf, view) in outs.items():
        _fence_intact(sent, buf, FENCE + shift, sizes[k], what + (k,))
    for k, (host, buf, view) in bufs.items():
        assert torch.equal(_bits(buf.cpu()), _bits(host)), what + (k, "an input was written")
    assert torch.equal(_bits(arena.data.cpu()), _bits(params_before)), what + ("the parameter block was written",)
    got["out"] = outs["out"][2].view(R, c.P, c.O)
    if hidden:
        got["hidden"] = outs["hidden"][2].view(c.layers, R, H)
    if saving:
        n_main = steps * c.layers * R * 6 * H
        got["save"] = outs["save"][2][:n_main].view(steps, c.layers, R, 6, H)
        got["dec"] = outs["save"][2][n_main:].view(c.P, R, 16 + H)
        if backward:
            n_main = steps * c.layers * R * 4 * H
            got["dsave"] = outs["dsave"][2][:n_main].view(steps, c.layers, R, 4, H)
            got["ddec"] = outs["dsave"][2][n_main:].view(c.P, R, 16)
    got["_keepalive"] = (bufs, outs, ins)
    return got


TENSORS = ("out", "hidden", "save", "dec", "dsave", "ddec")


def same_results(a, b, what, rows_a=None, rows_b=None):
    """every tensor both runs hold, bit for bit; rows_a / rows_b select the rows to compare"""
    for k in TENSORS:
        if k in a and k in b:
            ax = {"out": 0, "hidden": 1, "save": 2, "dec": 1, "dsave": 2, "ddec": 1}[k]
            x = a[k].cpu() if rows_a is None else a[k].cpu().index_select(ax, torch.as_tensor(rows_a))
            y = b[k].cpu() if rows_b is None else b[k].cpu().index_select(ax, torch.as_tensor(rows_b))
            _same(x, y, what + (k,))
    if "grads" in a and "grads" in b:
        for k in a["grads"]:
            _same(a["grads"][k], b["grads"][k], what + ("grad", k))


# ================================================================================================ the rule
def _rule(got, r64, r32, worst, key, what, own_scale):
    g, a, b = got.detach().cpu().double(), r64.double(), r32.double()
    assert g.shape == a.shape, (what, key, g.shape, a.shape)
    assert torch.isfinite(g).all(), (what, key, "not finite")
    assert not g[a == 0].any(), (what, key, "a cell that is exactly zero in fp64 is not zero")
    if not a.any():
        return
    if own_scale:
        err, e32 = _grad_err(g, a), _grad_err(b, a)
    else:
        scale = max(1.0, a.abs().max().item())
        err, e32 = (g - a).abs().max().item() / scale, (b - a).abs().max().item() / scale
    print(what, key, "err", err, "e32", e32, "bound", _bound(e32))
    group = key.split(".")[0]
    _worse(worst, group, err)
    _worse(worst, group + "_e32", e32)
    assert err <= _bound(e32), (what, key, err, e32, _bound(e32))


SAVE_FIELDS = ("h_prev", "r", "z", "n", "gh_n", "h_new")
DSAVE_FIELDS = ("dr", "dz", "dn_i", "dn_h")


def assert_vs_reference(c, got, r64, r32, worst, what):
    _rule(got["out"], r64["out"], r32["out"], worst, "out", what, False)
    if "hidden" in got:
        _rule(got["hidden"], r64["hidden"], r32["hidden"], worst, "hidden_out", what, False)
    if "save" in got:
        for f, name in enumerate(SAVE_FIELDS):
            _rule(got["save"][..., f, :], r64["save"][..., f, :], r32["save"][..., f, :], worst, "save." + name, what, False)
        _rule(got["dec"][..., :16], r64["dec"][..., :16], r32["dec"][..., :16], worst, "save.dec_in", what, False)
        _rule(got["dec"][..., 16:], r64["dec"][..., 16:], r32["dec"][..., 16:], worst, "save.act", what, False)
        assert not got["dec"][..., c.O:16].cpu().any(), (what, "columns >= O of the decoder-input block are not zero")
        assert not got["save"][0, :, :, 0].cpu().any(), (what, "h_prev of the first encoder step is not zero")
    if "dsave" in got:
        for stack, sl in (("enc", slice(0, c.T_in)), ("dec", slice(c.T_in, c.T_in + c.P))):
            for k in range(c.layers):
                for f, name in enumerate(DSAVE_FIELDS):
                    _rule(got["dsave"][sl, k, :, f], r64["dsave"][sl, k, :, f], r32["dsave"][sl, k, :, f], worst, f"dsave.{name}.{stack}{k}", what, True)
        _rule(got["ddec"], r64["ddec"], r32["ddec"], worst, "dsave.d_out", what, True)
        assert not got["ddec"][..., c.O:].cpu().any(), (what, "columns >= O of the d out block are not zero")
        if c.dropout == "keep" and c.rows > 1 and got["dsave"].shape[2] == c.rows:     # row 0: every flag 0, nothing of it reaches the loss
            assert not r64["dsave"][:, :, 0].any() and not got["dsave"][:, :, 0].cpu().any(), (what, "row gradients of a row with every flag 0")
            assert got["ddec"][:, 0, :c.O].cpu().any(), (what, "d out of a row with every flag 0 is the loss's own gradient, not zero")
    if "grads" in got:
        for k, v in got["grads"].items():
            _rule(v, r64["grads"][k], r32["grads"][k], worst, "grad." + k, what, True)


# ================================================================================================ the checks
def check_case(device, c):
    """the saving forward, the backward and the parameter gradients against fp64; 1: the non-saving forward gives the same ``out`` bits,
    with and without ``hidden_out``, and ``hidden_out`` is the h_new field of the last decoder step, layer by layer, bit for bit"""
    worst = {}
    what = (case_id(c),)
    got = launch(device, c, grads=True)
    assert_vs_reference(c, got, reference(c, torch.float64), reference(c, torch.float32), worst, what)
    _same(got["hidden"], got["save"][c.T_in + c.P - 1, :, :, 5], what + ("hidden_out is not the last step's h_new",))
    plain = launch(device, c, saving=False)
    _same(plain["out"], got["out"], what + ("the non-saving forward's out",))
    _same(plain["hidden"], got["hidden"], what + ("the non-saving forward's hidden_out",))
    bare = launch(device, c, saving=False, hidden=False)
    _same(bare["out"], got["out"], what + ("out without hidden_out",))
    return worst


def check_feedback_forms(device):
    """every feedback form against fp64 (FEEDBACK_CASES run through check_case); here the bit identities: a teacher whose coins are all
    0 is no teacher, and a teacher fed only after the last step feeds no step"""
    base = FEEDBACK_CASES[0]
    runs = {f: launch(device, base._replace(feedback=f), grads=True) for f in ("none", "zeros", "last")}
    same_results(runs["none"], runs["zeros"], ("no teacher", "coins all 0"))
    same_results(runs["zeros"], runs["last"], ("coins all 0", "only the last coin"))
    ones = launch(device, base._replace(feedback="ones"))
    assert not torch.equal(_bits(ones["out"].cpu()), _bits(runs["none"]["out"].cpu())), "teacher forcing changed nothing"
    return {}


def check_rows_independent(device, c=LARGEST, alone=ALONE):
    """2: a 129-row launch against the same rows alone (``alone``: every row on the GPU, ALONE on the emulator, where a one-row launch
    costs a workgroup's worth of emulated lanes), reversed, and as the 64-row and 65-row halves: out, hidden_out, each row's record and
    row gradients bit for bit -- a row's result depends on neither its workgroup, its wave nor its lane"""
    d = make_data(c)
    R = c.rows
    full = {k: v.cpu() for k, v in launch(device, c).items() if k in TENSORS}
    for r in alone:
        same_results(full, launch(device, c, take(d, [r])), ("row alone", r), rows_a=[r])
    rev = list(range(R - 1, -1, -1))
    same_results(full, launch(device, c, take(d, rev)), ("reversed",), rows_a=rev)
    for idx in (list(range(64)), list(range(64, R))):
        same_results(full, launch(device, c, take(d, idx)), ("half", idx[0]), rows_a=idx)
    return {}


def check_reads(device, c=_c(In=17, O=5, P=4, feedback="first")):
    """4: NaN in every float the contract does not own -- behind the last row of x, last, teacher, keep and g_out, in teacher[:, t]
    wherever coins[t] == 0 and at t = P - 1 -- changes no result bit; nor does a drop_p given without ``keep``"""
    for cc in (c, c._replace(feedback="ones"), c._replace(feedback="last", rows=17)):
        same_results(launch(device, cc, grads=True), launch(device, cc, pad=NAN, grads=True), ("NaN outside the extents", cc.feedback))
    nk = c._replace(dropout="none")
    same_results(launch(device, nk), launch(device, nk, drop_p_without_keep=True), ("drop_p without keep",))
    return {}


def check_misaligned(device, cases=(_c(In=17, O=5), _c(In=16, H=64, layers=1, O=16), _c(In=64, O=4, rows=17))):
    """5: every tensor base one float off its allocation -- x, last, teacher, keep, out, g_out, hidden_out, save and dsave take the
    scalar path of vload / vstore -- against fp64 by the rule, and bit for bit against the aligned run: the two paths move the same
    values, no arithmetic differs"""
    worst = {}
    for c in cases:
        got = launch(device, c, shift=1, pad=NAN)
        assert_vs_reference(c, got, reference(c, torch.float64), reference(c, torch.float32), worst, (case_id(c), "misaligned"))
        same_results(launch(device, c), got, (case_id(c), "aligned", "misaligned"))
    return worst


def check_repeatable(device, c=LARGEST, n=20):
    """6: ``n`` launches of the largest case give the same bits (twenty on the GPU; the emulator walks the lanes in one fixed order, so
    there a repeat can only show state that outlives a launch, and three do)"""
    first = launch(device, c, grads=True)
    for i in range(1, n):
        same_results(first, launch(device, c, grads=(i == n - 1)), ("launch", i))
    return {}


def check_refusals(device):
    """7: every condition of both launchers comes back as IPLAN_EINVAL with a message that names the entry point, and nothing is
    launched: the outputs keep their sentinels.  The restored descriptors launch."""
    lib = L.get_lib()
    EINVAL = _einval()
    c = _c(In=5, O=2, rows=17, feedback="ones")
    d = make_data(c)
    R = c.rows
    ins = {k: d[k].to(device) for k in ("x", "last", "teacher", "keep", "gw")}
    ins["coins"] = torch.tensor(coins_of(c), dtype=torch.int32).to(device)
    a = fill_args(device, c, d, ins)
    n_save, n_dsave = save_floats(R, c.T_in, c.P, c.layers, c.H)
    sizes = dict(out=R * c.P * c.O, hidden_out=c.layers * R * c.H, save=n_save, dsave=n_dsave)
    outs = {k: _sentinel(n, "cpu").to(device) for k, n in sizes.items()}
    a.out, a.hidden_out, a.save = (outs[k].data_ptr() for k in ("out", "hidden_out", "save"))
    b = L.Seq2SeqBwdArgs()
    b.g_out, b.dsave = ins["gw"].data_ptr(), outs["dsave"].data_ptr()
    count = 0

    def refused(name, **fields):
        nonlocal count
        fn = getattr(lib.c, name)
        if "null" in fields:
            rc = fn(None, C.c_void_p(0))
        else:
            old = {}
            for k, v in fields.items():
                if isinstance(v, tuple):                      # (index, value) of an offset array
                    old[k] = (v[0], getattr(a, k)[v[0]])
                    getattr(a, k)[v[0]] = v[1]
                elif hasattr(a, k):
                    old[k] = getattr(a, k)
                    setattr(a, k, v)
                else:
                    old[k] = getattr(b, k)
                    setattr(b, k, v)
            b.fwd = a
            rc = fn(C.byref(b if name.endswith("bwd") else a), C.c_void_p(L.current_stream(device) or 0))
            for k, v in old.items():
                if isinstance(v, tuple):
                    getattr(a, k)[v[0]] = v[1]
                elif hasattr(a, k):
                    setattr(a, k, v)
                else:
                    setattr(b, k, v)
            b.fwd = a
        msg = lib.c.iplan_last_error().decode()
        assert rc == EINVAL and rc < 0 and msg.startswith(name), (name, fields, rc, msg)
        count += 1

    for name in ("iplan_seq2seq_fwd", "iplan_seq2seq_bwd"):
        refused(name, null=True)
        for k, bad in (("rows", 0), ("T_in", 0), ("In", 0), ("In", 65), ("layers", 0), ("layers", 5), ("P", 0), ("O", 0), ("O", 17), ("H", 16), ("H", 48),
                       ("H", 128)):
            refused(name, **{k: bad})
        refused(name, params=None)
        for p in (-0.5, 1.0, 1.5, NAN):                                          # the backward divides by 1 - drop_p as well
            refused(name, drop_p=p)
        refused(name, teacher=None)                                               # coins without a teacher
        refused(name, coins=None)                                                 # a teacher that would be silently ignored
        refused(name, params=a.params + 4)                                        # weight_hh fragments are 16-byte loads
        for k in range(c.layers):
            refused(name, enc_off=(4 * k + 1, a.enc_off[4 * k + 1] + 1))
            refused(name, dec_off=(4 * k + 1, a.dec_off[4 * k + 1] + 2))
    for k in ("x", "last", "out"):
        refused("iplan_seq2seq_fwd", **{k: None})
    for k in ("save", "g_out", "dsave"):
        refused("iplan_seq2seq_bwd", **{k: None})
    _sync(device)
    for k, v in outs.items():
        assert torch.equal(_bits(v.cpu()), _bits(_sentinel(sizes[k], "cpu"))), (k, "a refused call wrote something")
    # what stays accepted: drop_p out of range WITHOUT keep (ignored, as the header says), unused layers' offsets unaligned
    stream = L.current_stream(device)
    keep_ptr, a.keep, a.drop_p = a.keep, None, 7.0
    a.enc_off[4 * c.layers + 1] = 3
    lib.call("iplan_seq2seq_fwd", a, stream)
    b.fwd = a
    lib.call("iplan_seq2seq_bwd", b, stream)
    a.keep, a.drop_p = keep_ptr, DROP_P
    lib.call("iplan_seq2seq_fwd", a, stream)
    b.fwd = a
    lib.call("iplan_seq2seq_bwd", b, stream)
    _sync(device)
    return {"refusals": count}
