"""Drop-in proof against the REAL reference objects, carried to every machine by tests/golden/reference_dropin.pt
(oracle/make_golden.py golden_reference_dropin records it where the reference tree exists): the episode the all-reference stack
produces in the reference's own ``ParallelRunner.run`` loop (runners/ippo_parallel_runner.py:105-281) and ``EpisodeBatch``, the
episode that loop produces driving the iplan_amd classes, the reference learners' parameters after one update on a
reference-filled episode, and the reference's value loss / returns under every loss switch.  The iplan_amd classes --
DcntrlMAC, Behavior_policy, Prediction_policy, IPPOLearner, host-emulated kernels -- and iplan_amd's runner, through a stub
vector env, are compared with them from the same weights on the same observation stream."""
import hashlib
import lzma
from functools import partial

import numpy as np
import pytest
import torch


class _Log:
    def __init__(self):
        self.stats = {}

    def log_stat(self, k, v, t):
        self.stats[k] = v


@pytest.fixture()
def emu():
    from iplan_amd import _lib as L
    from tests.emu.emu_lib import get_emu_lib
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


def _args(**kw):
    from iplan_amd.config import default_args
    K, nA, n_other, d = 3, 2, 5, 5            # ParallelRunner.action2env_tuple (:81-83) needs n_actions == n_agents (5 == 5 in Highway)
    a = default_args("highway", use_cuda=False, batch_size_run=K, n_agents=nA, n_other_vehicles=n_other, max_vehicle_num=n_other + nA,
                     episode_limit=6, max_history_len=3, buffer_size=K, batch_size=K - 1, ppo_epoch=2, pred_batch_size=4, pred_length=2,
                     n_obs_vehicles=4, device="cpu", animation_enable=False, n_actions=nA, **kw)
    a.obs_shape = a.obs_shape_single * a.n_obs_vehicles
    a.state_shape = a.obs_shape_single * a.max_vehicle_num
    return a


class _OneHot:
    """components/transforms.py:8-21 as far as the episode container needs it (the reference's own class when recording)"""

    def __init__(self, out_dim):
        self.out_dim = out_dim

    def infer_output_info(self, vshape_in, dtype_in):
        return (self.out_dim,), torch.float32


def _scheme_groups_preprocess(args, OneHot=_OneHot):
    from iplan_amd import synth
    scheme = synth.make_scheme(args)
    scheme.pop("actions_onehot")
    scheme.pop("filled")
    return scheme, {"agents": args.n_agents}, {"actions": ("actions_onehot", [OneHot(out_dim=args.n_actions)])}


def _env(args, seed=0, end_steps=None):
    from iplan_amd import synth
    return synth.StubHighwayVecEnv(args.batch_size_run, args.n_agents, args.n_obs_vehicles, args.obs_shape_single, args.max_vehicle_num,
                                   args.episode_limit, seed=seed, end_steps=end_steps, n_ids=args.max_vehicle_num - 2)


def _stack(args, ours):
    """(mac, behaviour, prediction, learner) from iplan_amd or from the reference, on the reference's scheme"""
    scheme, groups, _ = _scheme_groups_preprocess(args)
    full_scheme = dict(scheme, actions_onehot={"vshape": (args.n_actions,), "group": "agents", "dtype": torch.float32},
                       filled={"vshape": (1,), "dtype": torch.long})
    if ours:
        from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
        from iplan_amd.learners.ippo_learner import IPPOLearner
        from iplan_amd.nova.prediction_policy import Prediction_policy
        from iplan_amd.nova.stable_behavior_policy import Behavior_policy
    else:
        from controllers.dcntrl_controller import DcntrlMAC
        from learners.ippo_learner import IPPOLearner
        from nova.prediction_policy import Prediction_policy
        from nova.stable_behavior_policy import Behavior_policy
    log = _Log()
    mac = DcntrlMAC(full_scheme, groups, args)
    beh, pred = Behavior_policy(args, log), Prediction_policy(args, log)
    learner = IPPOLearner(mac, full_scheme, log, args)
    return mac, beh, pred, learner


NETS = (("mac", "agents"), ("mac", "critics"), ("beh", "behavior_encoder"), ("beh", "behavior_decoder"), ("pred", "pred_GAT"),
        ("pred", "pred_decoder"))


def _weights(stack):
    """{net family: [state dict per agent]} of a (mac, behaviour, prediction, learner) stack"""
    owner = dict(zip(("mac", "beh", "pred"), stack))
    return {name: [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in getattr(owner[o], name)] for o, name in NETS}


def _sha256(weights):
    """{family: [{name: sha256 of the tensor's dtype, shape and bytes}]}: the fixture's exact record of a set of weights"""
    return {name: [{k: hashlib.sha256(f"{v.dtype}{tuple(v.shape)}".encode() + v.detach().contiguous().numpy().tobytes()).hexdigest()
                    for k, v in sd.items()} for sd in ms] for name, ms in weights.items()}


def _pack(tensors):
    """{name: tensor} -> {"meta", "blob"}: the tensors' bytes, byte planes apart, LZMA-compressed (lossless; blob: uint8 tensor)"""
    meta, parts = [], []
    for k, t in tensors.items():
        a = t.detach().contiguous().numpy()
        meta.append((k, a.dtype.str, a.shape))
        parts.append(a.reshape(-1).view(np.uint8).reshape(-1, a.itemsize).T.tobytes())
    return dict(meta=meta, blob=torch.frombuffer(bytearray(lzma.compress(b"".join(parts), preset=9)), dtype=torch.uint8))


def _unpack(packed):
    raw, out, o = lzma.decompress(packed["blob"].numpy().tobytes()), {}, 0
    for k, dt, shape in packed["meta"]:
        dt = np.dtype(dt)
        n = int(np.prod(shape)) * dt.itemsize
        a = np.frombuffer(raw[o:o + n], np.uint8).reshape(dt.itemsize, -1).T.copy().view(dt).reshape(shape)
        out[k] = torch.from_numpy(a)
        o += n
    return out


def _post_deltas(before, after):
    """the update as exact float64 differences (after - before of two float32 tensors is exact in float64), packed"""
    return _pack({f"{name}.{i}.{k}": after[name][i][k].double() - v.double()
                  for name, ms in after.items() for i, sd in enumerate(before[name]) for k, v in sd.items()})


def _apply_deltas(before, packed):
    """the parameters after the update, bit for bit: ``before`` + the packed differences, rounded to float32"""
    d = _unpack(packed)
    return {name: [{k: (v.double() + d[f"{name}.{i}.{k}"]).to(v.dtype) for k, v in sd.items()} for i, sd in enumerate(before[name])]
            for name in {key.split(".")[0] for key in d}}


def _run_our_runner(args, stack, env):
    """iplan_amd.runners.ParallelRunner with its own episode container (never a reference class, even where one is importable)"""
    from iplan_amd.runners.ippo_parallel_runner import ParallelRunner, _dict_batch
    scheme, groups, preprocess = _scheme_groups_preprocess(args)
    runner = ParallelRunner(args, env, _Log())
    runner.setup(scheme, groups, preprocess, stack[0], stack[1], stack[2])
    runner.new_batch = partial(_dict_batch, scheme, groups, args.batch_size_run, args.episode_limit + 1, preprocess=preprocess, device="cpu")
    batch, *_ = runner.run(test_mode=False)
    return batch, runner


def test_reference_parallel_runner_drives_iplan_amd(golden, emu):
    """The reference's ParallelRunner.run + EpisodeBatch drove the iplan_amd classes when the fixture was recorded, and
    oracle/make_golden.py golden_reference_dropin asserted there what this test asserted with the reference present (the
    deterministic fields equal the all-reference run's, the learners take the reference's EpisodeBatch unchanged).  Here: the
    iplan_amd classes from the same weights, stepped in the reference runner's order from the same seeds, give the all-reference
    episode's deterministic fields; the learners then consume the episode container unchanged."""
    fixture = golden("reference_dropin")
    g = fixture["runner"]
    args = _args()
    torch.manual_seed(0)
    mine = _stack(args, ours=True)
    assert _sha256(_weights(mine)) == fixture["weights_sha256"]              # the reference stack's weights at this seed, exactly
    end = [args.episode_limit + 5, 4, args.episode_limit + 5]                 # env 1 terminates early
    torch.manual_seed(1)
    np.random.seed(1)
    b_mine, runner = _run_our_runner(args, mine, _env(args, 3, end))
    b_ref = _unpack(g["episode"])
    T1 = args.episode_limit + 1
    for k in ("history", "state", "obs", "reward", "terminated", "filled", "avail_actions", "speed"):
        assert torch.equal(b_mine[k], b_ref[k]), k
    # the behavioural incentive has no random draw on its path: identical up to fp32 round-off at every step
    assert (b_mine["behavior_latent"] - b_ref["behavior_latent"]).abs().max() < 1e-5
    assert b_mine["behavior_latent"].abs().sum() > 0 and b_mine["attention_latent"][:, 1:].abs().sum() > 0
    assert b_mine["actions"].shape == (args.batch_size_run, T1, args.n_agents, 1)
    assert torch.equal(b_mine["actions_onehot"].sum(-1)[:, :args.episode_limit], torch.ones(args.batch_size_run, args.episode_limit, args.n_agents))
    # step 0 has no sampled quantity upstream of the actor / critic except the gumbel gate of the first GAT update
    assert (b_mine["rnn_states_actors"][:, 0] - b_ref["rnn_states_actors_0"]).abs().max() == 0
    mac, beh, pred, learner = mine
    t_env = runner.t_env
    bl, sl, tl = beh.learn(b_mine, t_env)
    pl = pred.learn(b_mine, t_env)
    assert len(bl) == args.n_agents and len(pl) == args.n_agents and all(np.isfinite(float(x)) for x in list(bl) + list(pl))
    before = [p.detach().clone() for p in mac.agents[0].parameters()]
    learner.insert_episode_batch(b_mine)
    learner.train(t_env)
    assert any((a - b).abs().max() > 0 for a, b in zip(before, mac.agents[0].parameters()))


def test_learners_match_reference_on_a_reference_episode_batch(golden, emu):
    """One episode (filled by the reference's runner and stack, stored whole) through the iplan_amd learners: post-update
    parameters of the behaviour nets (injected dropout via a fixed in-kernel seed is not comparable, so dropout is 0 here) and of
    the PPO actors / critics agree, element for element, with the reference learners' on the same episode from the same weights."""
    from iplan_amd import synth
    fixture = golden("reference_dropin")
    g = fixture["learners"]
    args = _args(decoder_dropout=0.0)
    torch.manual_seed(0)
    mine = _stack(args, ours=True)
    before = _weights(mine)
    assert _sha256(before) == fixture["weights_sha256"]
    ref = _apply_deltas(before, g["post_deltas"])
    batch = synth.DictBatch(_unpack(g["episode"]), args.batch_size_run, args.episode_limit + 1)
    mine[1].learn(batch, 0)
    mine[3].insert_episode_batch(batch)
    mine[3].train(0)
    for i in range(args.n_agents):
        for name in ("behavior_encoder", "behavior_decoder"):
            for (k, a), (_, b) in zip(getattr(mine[1], name)[i].state_dict().items(), ref[name][i].items()):
                assert (a - b).abs().max() <= 1e-6 * max(1.0, b.abs().max().item()), (name, i, k)
        for a_m, a_r in ((mine[0].agents[i], ref["agents"][i]), (mine[0].critics[i], ref["critics"][i])):
            for (k, a), (_, b) in zip(a_m.state_dict().items(), a_r.items()):
                assert (a - b).abs().max() <= 1e-5 * max(1.0, b.abs().max().item()), (i, k, (a - b).abs().max().item())


def test_device_resident_runner_equals_reference_runner(golden, emu):
    """iplan_amd.runners.ParallelRunner (in-place launches into the episode container, one D2H of the actions per step) vs
    the reference's ParallelRunner driving the same iplan_amd classes from the same seeds: every field of the episode,
    sampled actions included; one env terminates early, so later steps store action 0 for it."""
    fixture = golden("reference_dropin")
    g = fixture["runner_vs_runner"]
    args = _args()
    torch.manual_seed(0)
    mine = _stack(args, ours=True)
    assert _sha256(_weights(mine)) == fixture["weights_sha256"]
    end = [args.episode_limit + 5, 3, args.episode_limit + 5]
    torch.manual_seed(4)
    np.random.seed(4)
    b_dev, r_dev = _run_our_runner(args, mine, _env(args, 7, end))
    b_ref = _unpack(g["episode"])
    assert r_dev.t_env == g["t_env"] and r_dev.t == g["t"]
    for k in ("actions", "actions_onehot", "filled", "terminated", "avail_actions"):
        assert torch.equal(b_dev[k], b_ref[k]), k
    for k in ("history", "state", "obs", "reward", "speed", "behavior_latent", "attention_latent", "rnn_states_actors", "rnn_states_critics"):
        assert (b_dev[k].float() - b_ref[k].float()).abs().max() <= 1e-6, (k, (b_dev[k].float() - b_ref[k].float()).abs().max().item())


def test_device_resident_runner_all_terminated_break(emu):
    """No reference tree needed: the built-in episode container; every env terminated -> the loop breaks like
    ippo_parallel_runner.py:212-214 and the trailing steps stay unfilled (actions 0, one-hot rows all zero)."""
    from iplan_amd import synth
    from iplan_amd.controllers.dcntrl_controller import DcntrlMAC
    from iplan_amd.nova.prediction_policy import Prediction_policy
    from iplan_amd.nova.stable_behavior_policy import Behavior_policy
    from iplan_amd.runners.ippo_parallel_runner import ParallelRunner, _dict_batch
    args = _args()
    scheme = synth.make_scheme(args)
    scheme.pop("actions_onehot")
    scheme.pop("filled")
    full = dict(scheme, actions_onehot={"vshape": (args.n_actions,), "group": "agents"}, filled={"vshape": (1,), "dtype": torch.long})
    mac = DcntrlMAC(full, {"agents": args.n_agents}, args)
    beh, pred = Behavior_policy(args, _Log()), Prediction_policy(args, _Log())
    runner = ParallelRunner(args, _env(args, 9, [3, 2, 3]), _Log())
    runner.setup(scheme, {"agents": args.n_agents}, {"actions": ("actions_onehot", [_OneHot(args.n_actions)])}, mac, beh, pred)
    runner.new_batch = lambda: _dict_batch(scheme, {"agents": args.n_agents}, args.batch_size_run, args.episode_limit + 1,
                                           {"actions": ("actions_onehot", [_OneHot(args.n_actions)])}, "cpu")
    batch, _, _, avg_len = runner.run()
    assert runner.t == 2 and float(batch["filled"].sum()) == 3 * args.batch_size_run
    assert batch["actions_onehot"][:, 3:].abs().sum() == 0 and batch["actions"][:, 3:].abs().sum() == 0
    assert torch.isfinite(batch["attention_latent"]).all() and batch["behavior_latent"][:, 2].abs().sum() > 0


def test_oracle_ppo_loss_switches_match_the_reference(golden):
    """oracle.ppo_losses / gae_returns with the loss switches off their shipped values == the reference's own
    cal_value_loss / compute_returns (learners/ippo_learner.py:128-159, 344-365) on the same inputs"""
    import itertools
    from oracle import iplan_oracle as O
    g = golden("reference_dropin")["ppo_losses"]
    values, vpred, rets, masks = g["values"], g["vpred"], g["rets"], g["masks"]
    zero = torch.zeros_like(values)
    for hub, clipv, act in itertools.product((True, False), repeat=3):
        want = g["value_loss"][(hub, clipv, act)]
        got = O.ppo_losses(zero, zero.mean(), values, zero, zero, vpred, rets, masks, 0.2, 10.0, 0.01, 0.5,
                           use_huber_loss=hub, use_clipped_value_loss=clipv, use_value_active_masks=act)[3]
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-7), (hub, clipv, act, float(got), float(want))
    for use_gae in (True, False):
        want = g["returns"][use_gae]
        got = O.gae_returns(g["rewards"], g["v_all"].unsqueeze(-1), g["terminated"], 0.99, 0.95, use_gae=use_gae)
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-6), use_gae
