"""DcntrlMAC -- decentralised multi-agent controller without parameter sharing (mirror of
controllers/dcntrl_controller.py:9-232).

Same constructor and method contracts as the reference.  Differences are internal:
  * the n_agents private R_Actor / R_Critic modules keep their own ``state_dict`` (checkpoints
    interchange with the reference) but their weights live in two stacked arenas, so
    ``select_actions_ippo`` is ONE fused launch for all agents, actors and critics, instead of
    2 * n_agents module calls;
  * the observation assembly of ``_build_inputs`` happens inside the kernel -- the [E, nA, F]
    input tensor is never materialised.  ``_build_inputs`` / ``_build_inputs_ippo`` remain available
    (plain tensor plumbing) for callers that want the assembled tensor.
"""
import copy
from types import SimpleNamespace

import numpy as np
import torch as th

from .. import ops
from ..arena import ParamArena
from ..modules.agents.ippo_actor import R_Actor
from ..modules.critics.ippo_critic import R_Critic


def _esn(t):
    """(net, chain, step) strides of a [E, S, nA, ...] tensor"""
    return (t.stride(2), t.stride(0), t.stride(1))


class DcntrlMAC:
    def __init__(self, scheme, groups, args):
        self.n_agents = args.n_agents
        self.args = args
        self.device = th.device("cuda" if args.use_cuda else "cpu")
        input_shape = self._get_input_shape(scheme)
        self.input_shape = input_shape
        self._build_agents(input_shape)
        self._build_critics(input_shape)
        self.actor_arena = ParamArena(self.agents, self.device)
        self.critic_arena = ParamArena(self.critics, self.device)
        # actor + critic gradients in ONE buffer: a data-parallel PPO step exchanges them as one collective (15 per train()
        # instead of 30; the exchange is latency-bound)
        ParamArena.colocate_grads([self.actor_arena, self.critic_arena])
        for i in range(self.n_agents):
            self.agents[i].attach(self.actor_arena, i)
            self.critics[i].attach(self.critic_arena, i)
        self.fc1_pack = ops.Fc1Pack(self.actor_arena, self.critic_arena)     # fragment-major fc1 operands, repacked when stale
        self.agent_output_type = args.agent_output_type
        self.hidden_states = None
        self.input_scheme = scheme

    # ------------------------------------------------------------------------------ IPPO
    def _widths(self):
        a = self.args
        src = [("history", a.obs_shape_single)]
        if a.GAT_enable:
            src.append(("attention_latent", a.attention_dim))
        if a.Behavior_enable:
            src.append(("behavior_latent", a.latent_dim))
        return src

    def _dev(self, t, dtype=None):
        t = t.to(self.device) if t.device != self.device else t
        return t if dtype is None or t.dtype == dtype else t.to(dtype)

    def select_actions_ippo(self, ep_batch, t_ep, test_mode=False, q_noise=None, as_numpy=True, write_back=False, phase_clocks=None, launch=True):
        """One fused launch: features gathered in place from ``ep_batch`` at ``t_ep``, all agents,
        actor + critic (controllers/dcntrl_controller.py:27-58).  Returns the reference's 5-tuple
        (values [E,nA], actions [E,nA], list of nA logp [E,1], rnn_states_actors [1,E,nA,M],
        rnn_states_critics [1,E,nA,M]); numpy for the array items unless ``as_numpy=False``.
        ``write_back=True`` (device-resident rollouts): the kernel additionally writes the actions, their
        one-hot and the new GRU states straight into ``ep_batch`` (actions / actions_onehot at ``t_ep``, rnn
        states at ``t_ep + 1``), i.e. the ``EpisodeBatch.update`` of ippo_parallel_runner.py:260-266.
        ``launch=False`` (with ``write_back``): nothing is enqueued; returns the prepared launch for
        ``Prediction_policy.GAT_latent_update(..., fuse_ac=...)`` of step ``t_ep - 1``, whose launch then carries this action
        selection behind the latent updates it reads (ops.gat_forward)."""
        a = self.args
        nA, N, M = self.n_agents, a.max_vehicle_num, a.rnn_hidden_dim
        E = ep_batch.batch_size
        sources = []
        for key, w in self._widths():
            full = self._dev(ep_batch[key], th.float32)                  # [E, T1, nA, N, w]
            view = full[:, t_ep]
            sources.append((view, w, view.stride(1), view.stride(0)))
        last = None
        la_strides = (0, 0)
        if a.obs_last_action and t_ep > 0:
            last = self._dev(ep_batch["actions"])[:, t_ep - 1, :, 0]             # [E, nA] int64 view, read in place
            la_strides = (last.stride(1), last.stride(0))
        spec = ops.AcFeatureSpec(N, sources, n_actions=a.n_actions if a.obs_last_action else 0,
                                 last_action=last, la_strides=la_strides,
                                 n_id=nA if a.obs_agent_id else 0, T=E, T_phys=E)
        assert spec.F == self.input_shape, (spec.F, self.input_shape)
        avail = self._dev(ep_batch["avail_actions"])[:, t_ep]            # [E, nA, n_act] int32 view
        if avail.dtype != th.int32:
            avail = avail.to(th.int32)
        ha = self._dev(ep_batch["rnn_states_actors"], th.float32)[:, t_ep]       # [E, nA, M]
        hc = self._dev(ep_batch["rnn_states_critics"], th.float32)[:, t_ep]
        assert ha.stride() == hc.stride()
        if not test_mode and q_noise is None:
            q_noise = th.empty(nA, E, a.n_actions, dtype=th.float32, device=self.device).exponential_()
        wb = {}
        if write_back:
            ha_n = ep_batch["rnn_states_actors"][:, t_ep + 1]             # [E, nA, M] views
            hc_n = ep_batch["rnn_states_critics"][:, t_ep + 1]
            act_n = ep_batch["actions"][:, t_ep, :, 0]
            oh_n = ep_batch["actions_onehot"][:, t_ep]
            assert ha_n.stride() == hc_n.stride()
            wb = dict(h_out=(ha_n, hc_n, (ha_n.stride(1), ha_n.stride(0))),
                      actions_out=(act_n, (act_n.stride(1), act_n.stride(0))),
                      onehot_out=(oh_n, (oh_n.stride(1), oh_n.stride(0))))
        o = ops.ac_forward(self.actor_arena, self.critic_arena, 2, spec, E, nA, h_actor=ha, h_critic=hc,
                           h_strides=(ha.stride(1), ha.stride(0)), avail=avail,
                           avail_strides=(avail.stride(1), avail.stride(0)),
                           mode=0 if test_mode else 1, q_noise=q_noise, n_actions=a.n_actions, phase_clocks=phase_clocks,
                           packed=self.fc1_pack.get(spec, fold=E <= 512), launch=launch, **wb)
        if not launch:
            assert write_back
            return o
        values = o["values"].t()                                          # [E, nA]
        logps = [o["logp"][i].reshape(E, 1) for i in range(nA)]
        if write_back:
            actions, ha_new, hc_new = act_n, ha_n.unsqueeze(0), hc_n.unsqueeze(0)
        else:
            actions = o["actions"].t()
            ha_new = o["h_actor"].permute(1, 0, 2).unsqueeze(0)           # [1, E, nA, M]
            hc_new = o["h_critic"].permute(1, 0, 2).unsqueeze(0)
        if as_numpy:
            return (values.cpu().numpy(), actions.cpu().numpy(), logps,
                    ha_new.cpu().numpy(), hc_new.cpu().numpy())
        return values, actions, logps, ha_new, hc_new

    # ------------------------------------------------------------------------------ inspection
    POLICY_STATS = ("weight", "entropy", "greedy_is_recorded", "logp", "value", "max_prob")

    def _rows(self, batch, t0, S):
        """The rows the policy saw at steps t0 .. t0 + S - 1 of a recorded ``batch`` (fields [E, T1, nA, ...], torch or numpy), read
        in place: the feature spec (row (e, s) at physical row e * T1 + t0 + s; the last action is the recorded one of t - 1, none
        at t = 0), the int32 ``avail`` and int64 ``acts`` [E, S, nA] of those steps, the packed fc1 operands, and the accessors
        ``dev`` (anything -> this device) and ``field`` (a batch field, each fetched once)."""
        a = self.args
        fields = {}

        def dev(t, dtype=None):
            return self._dev(th.as_tensor(t), dtype)

        def field(key, dtype=None):
            """[E, T1, ...] on the device, rows addressable as e * T1 + t (a copy only when the batch's layout is not that)"""
            if (key, dtype) not in fields:
                t = dev(batch[key], dtype)
                fields[key, dtype] = t if t.stride(0) == t.shape[1] * t.stride(1) and t[0, 0].is_contiguous() else t.contiguous()
            return fields[key, dtype]

        hist = field("history", th.float32)
        E, T1 = hist.shape[:2]
        assert 0 <= t0 and S >= 1 and t0 + S <= T1, (t0, S, T1)
        sl = slice(t0, t0 + S)
        sources = []
        for key, w in self._widths():
            view = (hist if key == "history" else field(key, th.float32))[:, sl]                  # [E, S, nA, N, w]
            sources.append((view, w, view.stride(2), view.stride(1)))
        acts = field("actions")[..., 0]                                                           # [E, T1, nA] int64
        last, la_strides = None, (0, 0)
        if a.obs_last_action:
            last = th.cat([th.full_like(acts[:, :1], -1), acts[:, :-1]], 1)[:, sl]                # the action of t - 1; none at t = 0
            la_strides = (last.stride(2), last.stride(1))
        spec = ops.AcFeatureSpec(a.max_vehicle_num, sources, n_actions=a.n_actions if a.obs_last_action else 0, last_action=last,
                                 la_strides=la_strides, n_id=self.n_agents if a.obs_agent_id else 0, T=S, T_phys=T1)
        assert spec.F == self.input_shape, (spec.F, self.input_shape)
        avail = field("avail_actions")
        if avail.dtype != th.int32:
            avail = avail.to(th.int32)
        return SimpleNamespace(spec=spec, E=E, T1=T1, sl=sl, avail=avail[:, sl], acts=acts[:, sl], dev=dev, field=field,
                               as_np=isinstance(batch["history"], np.ndarray), packed=self.fc1_pack.get(spec))

    def _target(self, r, target):
        """``target`` of saliency / saliency_trace -> (a* per row, int64 [E, S, nA], or None = every row's greedy action; its strides)"""
        if isinstance(target, str):
            assert target in ("recorded", "greedy"), target
            tgt = r.acts if target == "recorded" else None
        else:
            tgt = r.dev(target, th.int64)
            assert tgt.shape == r.acts.shape, (tgt.shape, tuple(r.acts.shape))
        return tgt, _esn(tgt) if tgt is not None else (0, 0, 0)

    def _trace(self, batch, t0, S, hidden0, which, want, want_h, rows=None):
        """ops.policy_trace over steps t0 .. t0 + S - 1 of ``batch``, fields read in place -> ([nA, E, S, ..] results, as_numpy,
        the recorded actions); ``rows``: ``_rows(batch, t0, S)`` where the caller has it already"""
        a = self.args
        if a.layer_N != 1 or a.recurrent_N != 1:
            raise NotImplementedError("policy_trace / action_distribution cover layer_N = recurrent_N = 1 only")
        nA, M = self.n_agents, a.rnn_hidden_dim
        r = rows if rows is not None else self._rows(batch, t0, S)
        E, avail, acts = r.E, r.avail, r.acts
        if isinstance(hidden0, str):
            assert hidden0 == "zeros", hidden0
            ha = hc = None
            hs = (0, 0)
        else:
            if hidden0 is None:
                ha, hc = r.field("rnn_states_actors", th.float32)[:, t0], r.field("rnn_states_critics", th.float32)[:, t0]
            else:
                ha, hc = (r.dev(h, th.float32) for h in hidden0)
            assert ha.shape == hc.shape == (E, nA, M), (ha.shape, hc.shape)
            if ha.stride() != hc.stride() or ha.stride(2) != 1:
                ha, hc = ha.contiguous(), hc.contiguous()
            hs = (ha.stride(1), ha.stride(0))
        w = {"actor": 0, "critic": 1, "both": 2}[which]
        want = tuple(k for k in want if (k == "values" and w != 0) or (k != "values" and w != 1))
        if want_h:
            want += tuple(k for k, on in (("h_actor", w != 1), ("h_critic", w != 0)) if on)
        res = ops.policy_trace(self.actor_arena, self.critic_arena, w, r.spec, E, S, nA, hidden0_actor=ha, hidden0_critic=hc, h_strides=hs,
                               avail=avail, avail_strides=(avail.stride(2), avail.stride(1)),
                               actions_in=acts if "logp" in want else None, act_strides=(acts.stride(2), acts.stride(1)),
                               n_actions=a.n_actions, want=want, packed=r.packed)
        return res, r.as_np, acts

    def policy_trace(self, batch, hidden0=None, which="both", want=("probs", "entropy", "greedy", "logp", "values", "stats"), return_hidden=False):
        """What would these actors and critics have done on a recorded episode batch, step by step?  ``batch``: what
        ``IPPOLearner.insert_episode_batch`` takes (fields [E, S, nA, ...], torch or numpy).  The nets walk the S steps with THEIR
        OWN GRU state, carried inside one pair of launches (ops.policy_trace); step s sees what the rollout showed the policy at
        t_ep = s: history / attention_latent / behavior_latent of step s (as GAT_enable / Behavior_enable say), the one-hot of the
        recorded ``actions[:, s-1]`` (zeros at s = 0; obs_last_action), the agent id (obs_agent_id) and ``avail_actions[:, s]``.
        ``hidden0``: None = the batch's ``rnn_states_actors[:, 0]`` / ``rnn_states_critics[:, 0]``, "zeros", or a pair of
        [E, nA, M] tensors.  ``which``: "actor", "critic" or "both".  Returns a dict with those of ``want`` the nets provide:
          probs [E,S,nA,n_actions] (unavailable actions exactly 0); entropy, logp (of the recorded ``actions[:, s]``), values
          [E,S,nA]; greedy [E,S,nA] int64 (argmax of probs, lowest index on ties);
          h_actor / h_critic [E,nA,M], the state after the last step -- [E,S,nA,M], after every step, with ``return_hidden``;
          stats [nA,S,6] float64 (which = "both" only): sums over the environments with weight ``batch["filled"][:, s]`` of
          POLICY_STATS = (the weight, entropy, 1[greedy == recorded action], logp, value, largest probability), formed on the
          device in float64 from the per-row outputs, in environment order.
        Device tensors in -> device tensors out, numpy in -> numpy out.  Draws from no generator; parameters, optimiser state,
        ``hidden_states`` and the batch are not touched.  Not covered: a free-running replay that feeds the policy's own greedy
        action back as the last action (the last action is always the recorded one), GAE / explained variance on the traced
        values, and layer_N / recurrent_N other than 1."""
        want = tuple(want)
        known = ("probs", "entropy", "greedy", "logp", "values", "stats")
        assert all(k in known for k in want), want
        stats = "stats" in want
        if stats and which != "both":
            raise ValueError('policy_trace: "stats" needs which="both" (its columns come from the actors and the critics)')
        S = batch["history"].shape[1]
        need = known[:5] if stats else tuple(k for k in want if k != "stats")
        res, as_np, acts = self._trace(batch, 0, S, hidden0, which, need, return_hidden)
        out = {}
        for k in want:
            if k in res:
                out[k] = res[k].permute(1, 2, 0, 3) if k == "probs" else res[k].permute(1, 2, 0)
        for k in ("h_actor", "h_critic"):
            if "h_last_" + k[2:] in res:
                out[k] = res[k].permute(1, 2, 0, 3) if return_hidden else res["h_last_" + k[2:]].permute(1, 0, 2)
        if stats:
            filled = batch["filled"]
            wt = self._dev(th.as_tensor(filled) if isinstance(filled, np.ndarray) else filled).reshape(-1, S).to(th.float64)     # [E, S]
            cols = th.stack([th.ones_like(res["entropy"]), res["entropy"], (res["greedy"] == acts.permute(2, 0, 1)).to(th.float32), res["logp"],
                             res["values"], res["probs"].max(-1).values], -1).to(th.float64)                                 # [nA, E, S, 6]
            tot = th.zeros(self.n_agents, S, len(self.POLICY_STATS), dtype=th.float64, device=self.device)
            for e in range(cols.shape[1]):                                        # environment order
                tot += cols[:, e] * wt[e][None, :, None]
            out["stats"] = tot
        return {k: v.cpu().numpy() for k, v in out.items()} if as_np else out

    def action_distribution(self, ep_batch, t_ep):
        """The distribution ``select_actions_ippo(ep_batch, t_ep)`` samples from, which it never returns: one step of
        ``policy_trace`` from the stored states ``rnn_states_*[:, t_ep]``.  Returns a dict: probs [E,nA,n_actions], greedy [E,nA]
        int64, entropy [E,nA], values [E,nA] (device tensors in -> device tensors out, numpy in -> numpy out)."""
        res, as_np, _ = self._trace(ep_batch, t_ep, 1, None, "both", ("probs", "greedy", "entropy", "values"), False)
        out = {k: res[k][:, :, 0].transpose(0, 1) for k in ("probs", "greedy", "entropy", "values")}
        return {k: v.cpu().numpy() for k, v in out.items()} if as_np else out

    def saliency(self, batch, target="recorded", which="both", hidden=None, want=("entity",), steps=None):
        """Which vehicles, and which of their inputs, drive this agent's decision and this critic's value?  The gradient of the actors'
        log-probability log pi(a* | x) and of the critics' value V(x) with respect to the INPUT row x = [hist || att || beh per entity,
        one-hots], one launch for all agents and rows (ops.saliency), reduced per entity and per source.  ``batch``: what
        ``policy_trace`` takes (fields [E, S, nA, ...], torch or numpy); step s sees exactly the inputs ``policy_trace`` shows it: the
        fields of step s, the recorded ``actions[:, s-1]`` as last action (none at s = 0), ``avail_actions[:, s]``.
        The GRU state of row (e, s) is the RECORDED ``rnn_states_actors[:, s]`` / ``rnn_states_critics[:, s]``, or, with
        ``hidden=(ha, hc)``, a pair of [E, S, nA, M] tensors over the selected steps.  The state is an input: it is held constant and
        nothing is differentiated through time (no BPTT), so a row's gradient is the sensitivity of THIS step's output to THIS step's
        observation.  ``target``: "recorded" (``actions[:, s]``), "greedy" (the row's own argmax, lowest index on ties) or an int tensor
        [E, S, nA] (-1 = greedy for that row).  ``steps``: None = every step, a slice with step 1, or an int = that one step, returned
        without the step axis (with an EpisodeBatch: the one-step form at t_ep).  ``which``: "actor", "critic" or "both".
        Returns a dict, [E, S, nA, ...] each:
          actor_gxi, critic_gxi [.., N, n_src]  sum_k g_k x_k over the source's columns of the entity (signed gradient x input)
          actor_gl1, critic_gl1 [.., N, n_src]  sum_k |g_k| over the same columns
          logp, values, target_action           y of the actors / critics and the a* that was used (int64)
          sources                               the tuple of field names, the n_src axis in ``_widths()`` order
          actor_input_grad, critic_input_grad [.., F]  with "input_grad" in ``want``: the whole gradient in the reference's column order
          actor_act1, actor_act2, critic_act1, critic_act2 [.., M]  with "act" in ``want``: the trunk's post-activation values (tests)
        Device tensors in -> device tensors out, numpy in -> numpy out.  Draws from no generator; parameters, gradient entries,
        optimiser state, ``hidden_states`` and the batch are not touched; the packed fc1 operands are brought up to date exactly as
        ``policy_trace`` does it (the values any later launch would pack), the kernel only reads them.  Not covered: layer_N /
        recurrent_N other than 1.  Back to the raw history: hand the ``beh`` columns of ``actor_input_grad`` to
        ``Behavior_policy.latent_saliency`` and the ``att`` columns to ``Prediction_policy.attention_saliency`` as ``target``;
        through time: ``saliency_trace``."""
        a = self.args
        if a.layer_N != 1 or a.recurrent_N != 1:
            raise NotImplementedError("saliency covers layer_N = recurrent_N = 1 only")
        want = tuple(want)
        assert all(k in ("entity", "input_grad", "act") for k in want), want
        nA, M = self.n_agents, a.rnn_hidden_dim
        T1 = batch["history"].shape[1]
        one = isinstance(steps, (int, np.integer))
        if steps is None:
            t0, S = 0, T1
        elif one:
            t0, S = int(steps), 1
        else:
            t0, t1, stride = steps.indices(T1)
            assert stride == 1, "steps: a slice with step 1"
            S = t1 - t0
        r = self._rows(batch, t0, S)
        E, as_np = r.E, r.as_np
        if hidden is None:
            ha, hc = r.field("rnn_states_actors", th.float32)[:, r.sl], r.field("rnn_states_critics", th.float32)[:, r.sl]
        else:
            ha, hc = (r.dev(h, th.float32) for h in hidden)
        assert ha.shape == hc.shape == (E, S, nA, M), (ha.shape, hc.shape, (E, S, nA, M))
        if ha.stride() != hc.stride() or ha.stride(3) != 1:
            ha, hc = ha.contiguous(), hc.contiguous()
        tgt, tgt_strides = self._target(r, target)
        w = {"actor": 0, "critic": 1, "both": 2}[which]
        res = ops.saliency(self.actor_arena, self.critic_arena, w, r.spec, E, S, nA, h_actor=ha, h_critic=hc, h_strides=_esn(ha),
                           avail=r.avail, avail_strides=_esn(r.avail), target=tgt, target_strides=tgt_strides, target_all=-1,
                           n_actions=a.n_actions, want=("y",) + want, packed=r.packed)
        out = {"sources": tuple(k for k, _ in self._widths())}
        for k in ("logp", "values", "target_action"):
            if k in res:
                out[k] = res[k].permute(1, 2, 0)
        for net in ("actor", "critic"):
            if "entity_" + net in res:
                ent = res["entity_" + net].permute(1, 2, 0, 3, 4, 5)                              # [E, S, nA, N, n_src, 2]
                out[net + "_gxi"], out[net + "_gl1"] = ent[..., 0], ent[..., 1]
            for k in ("input_grad", "act1", "act2"):
                if k + "_" + net in res:
                    out[net + "_" + k] = res[k + "_" + net].permute(1, 2, 0, 3)
        if one:
            out = {k: (v if k == "sources" else v[:, 0]) for k, v in out.items()}
        return {k: (v if k == "sources" else v.cpu().numpy()) for k, v in out.items()} if as_np else out

    def saliency_trace(self, batch, lags, target="recorded", which="both", hidden0=None, steps=None, want=("entity",)):
        """How far back does this policy look, and at whom?  ``saliency`` through time: the total derivative of the output of step s,
        y_s = log pi(a*_s | x_s, h_{s-1}) of the actors / V(x_s, h_{s-1}) of the critics, with respect to the INPUT row of step s - k,
        g_s^(k) = d y_s / d x_{s-k}, k = 0 .. ``lags``, through the recurrent state (BPTT over the GRU chain, truncated at ``lags``).
        The chain is the one ``policy_trace`` walks: h_s = GRU(trunk(x_s), h_{s-1}) with THESE nets' own states (the GRU output before
        rnn.norm), from ``hidden0`` -- None = the batch's ``rnn_states_actors[:, t0]`` / ``rnn_states_critics[:, t0]``, "zeros", or a
        pair of [E, nA, M] tensors -- traced first (ops.policy_trace); ``lags + 1`` launches follow (ops.saliency_lag), lag k seeded
        with d y_s / d h_{s-k}, the carry lag k - 1 left.  ``batch``, ``target`` and ``which`` as for ``saliency``.  ``steps``: None =
        every step, or a slice with step 1: the inspected window [t0, t0 + S); the chain starts at t0 and lags reaching before it do
        not exist.  ``lags``: an int in [0, S - 1]; S - 1 is full BPTT over the window.  Anything else raises ValueError.
        Returns a dict:
          actor_gxi, actor_gl1, critic_gxi, critic_gl1 [E, S, K+1, nA, N, n_src]  entry [e, s, k]: what the inputs of step s - k
                                    contribute to the output of step s (sum g x and sum |g| per entity and source); exactly 0 where s < k
          lag_valid [S, K+1] bool   s >= k
          actor_carry_l2, critic_carry_l2 [E, S, K+1, nA]  the 2-norm of d y_s / d h_{s-k-1}: what still flows into the state beyond lag k
          actor_lag_l1, critic_lag_l1 [nA, K+1] float64  the mean over e and s >= k, with weight ``batch["filled"][e, s]``, of the row's
                                    sum over entities and sources of gl1 (0 where the weights sum to 0); formed on the device in
                                    float64, in environment order, from the per-row outputs: the "how far back" curve
          logp, values, target_action [E, S, nA]; sources   as ``saliency``
          h_actor, h_critic [E, S, nA, M]  the traced states (after every step)
          actor_input_grad, critic_input_grad [E, S, K+1, nA, F]  with "input_grad" in ``want``
          actor_act1, actor_act2, critic_act1, critic_act2 [E, S, nA, M]  with "act" in ``want`` (tests)
          actor_carry, critic_carry [E, S, K+1, nA, M]  with "carry" in ``want``: d y_s / d h_{s-k-1} itself
        Device tensors in -> device tensors out, numpy in -> numpy out.  Draws from no generator; parameters, gradient entries,
        optimiser state, ``hidden_states`` and the batch are not touched.  Not covered: layer_N / recurrent_N other than 1.  Back to
        the raw history: ``Behavior_policy.latent_saliency`` (the ``beh`` columns) and ``Prediction_policy.attention_saliency`` (the
        ``att`` columns)."""
        a = self.args
        if a.layer_N != 1 or a.recurrent_N != 1:
            raise NotImplementedError("saliency_trace covers layer_N = recurrent_N = 1 only")
        want = tuple(want)
        assert all(k in ("entity", "input_grad", "act", "carry") for k in want), want
        nA, M = self.n_agents, a.rnn_hidden_dim
        T1 = batch["history"].shape[1]
        if steps is None:
            t0, S = 0, T1
        else:
            if not isinstance(steps, slice):
                raise ValueError("saliency_trace: steps is None or a slice with step 1")
            t0, t1, stride = steps.indices(T1)
            if stride != 1 or t1 - t0 < 1:
                raise ValueError("saliency_trace: steps is a non-empty slice with step 1")
            S = t1 - t0
        if isinstance(lags, bool) or not isinstance(lags, (int, np.integer)) or not 0 <= lags < S:
            raise ValueError(f"saliency_trace: lags={lags!r} is not an int in [0, {S - 1}]")
        K1 = int(lags) + 1
        r = self._rows(batch, t0, S)                                                              # the rows, as saliency() describes them
        E, as_np, dev = r.E, r.as_np, r.dev
        # 1: the chain from hidden0, and the state entering every step: cat(hidden0, h[:, :-1])
        w = {"actor": 0, "critic": 1, "both": 2}[which]
        tr, _, _ = self._trace(batch, t0, S, hidden0, which, (), True, rows=r)
        enter = {}
        for k, (net, on) in enumerate((("actor", w != 1), ("critic", w != 0))):
            if not on:
                continue
            if isinstance(hidden0, str):
                h0 = th.zeros(nA, E, 1, M, dtype=th.float32, device=self.device)
            elif hidden0 is None:
                h0 = r.field("rnn_states_" + net + "s", th.float32)[:, t0].permute(1, 0, 2).unsqueeze(2)
            else:
                h0 = dev(hidden0[k], th.float32).permute(1, 0, 2).unsqueeze(2)
            enter[net] = th.cat([h0, tr["h_" + net][:, :, :-1]], 2)                                # [nA, E, S, M], contiguous
        tgt, tgt_strides = self._target(r, target)
        any_h = enter["actor" if w != 1 else "critic"]
        # 2: lags + 1 launches
        res = ops.saliency_lag(self.actor_arena, self.critic_arena, w, r.spec, E, S, nA, K1 - 1, h_actor=enter.get("actor"),
                               h_critic=enter.get("critic"), h_strides=(any_h.stride(0), any_h.stride(1), any_h.stride(2)), avail=r.avail,
                               avail_strides=_esn(r.avail), target=tgt, target_strides=tgt_strides, target_all=-1, n_actions=a.n_actions,
                               want=("y", "entity") + tuple(k for k in want if k in ("input_grad", "act")), packed=r.packed)
        lag_valid = th.arange(S, device=self.device)[:, None] >= th.arange(K1, device=self.device)[None, :]        # [S, K+1]
        out = {"sources": tuple(k for k, _ in self._widths()), "lag_valid": lag_valid}
        for k in ("logp", "values", "target_action"):
            if k in res:
                out[k] = res[k].permute(1, 2, 0)
        filled = dev(batch["filled"]).reshape(-1, T1)[:, r.sl].to(th.float64)                    # [E, S]
        for net in enter:
            out["h_" + net] = tr["h_" + net].permute(1, 2, 0, 3)
            ent = res["entity_" + net]                                                            # [nA, E, S, K+1, N, n_src, 2]
            if "entity" in want:
                pe = ent.permute(1, 2, 3, 0, 4, 5, 6)
                out[net + "_gxi"], out[net + "_gl1"] = pe[..., 0], pe[..., 1]
            carry = res["carry_" + net]                                                           # [nA, E, S, K+1, M]; 0 where s < k
            out[net + "_carry_l2"] = carry.to(th.float64).pow(2).sum(-1).sqrt().to(th.float32).permute(1, 2, 3, 0)
            if "carry" in want:
                out[net + "_carry"] = carry.permute(1, 2, 3, 0, 4)
            row = ent[..., 1].to(th.float64).sum((-1, -2))                                        # [nA, E, S, K+1]
            wt = filled[:, :, None] * lag_valid                                                   # [E, S, K+1]
            per_env = th.cat([(row * wt).sum(2), wt.sum(1)[None]])                                # [nA + 1, E, K+1]: weighted sums | weights
            tot = th.zeros(nA + 1, K1, dtype=th.float64, device=self.device)
            for e in range(E):                                                                    # environment order
                tot += per_env[:, e]
            num, den = tot[:nA], tot[nA]
            out[net + "_lag_l1"] = th.where(den > 0, num / den.clamp_min(1e-300), th.zeros_like(num))
            if "input_grad" in want:
                out[net + "_input_grad"] = res["input_grad_" + net].permute(1, 2, 3, 0, 4)
            if "act" in want:
                for k in ("act1", "act2"):
                    out[net + "_" + k] = res[k + "_" + net].permute(1, 2, 0, 3)
        return {k: (v if k == "sources" else v.cpu().numpy()) for k, v in out.items()} if as_np else out

    # ---- what knockout() and knockout_trace() share; ``name`` is the method's, for the messages
    def _knock_request(self, name, want, entities, sources, which, presence_col, max_workspace_mb, **dicts):
        """the arguments both methods validate alike -> (want, the entity list, the knocked source names, ``_widths()``)"""
        a = self.args
        if a.layer_N != 1 or a.recurrent_N != 1:
            raise NotImplementedError(f"{name} covers layer_N = recurrent_N = 1 only")
        want, allowed = tuple(want), getattr(self, name.upper() + "_WANT")
        if any(k not in allowed for k in want):
            raise ValueError(f"{name}: want={want!r} names something other than {allowed}")
        if which not in ("actor", "critic", "both"):
            raise ValueError(f"{name}: which={which!r}")
        N, widths = a.max_vehicle_num, self._widths()
        names = [k for k, _ in widths]
        ents = list(range(N)) if entities is None else [int(j) for j in np.asarray(entities).reshape(-1)]
        if not ents or any(not -1 <= j < N for j in ents):
            raise ValueError(f"{name}: entities={ents!r} must be a non-empty list of indices in [-1, {N})")
        srcs = tuple(names) if sources is None else tuple(sources)
        if not srcs or any(k not in names for k in srcs):
            raise ValueError(f"{name}: sources={srcs!r} is not a non-empty subset of {names!r}")
        for what, d in dicts.items():
            if d is not None and (not isinstance(d, dict) or any(k not in names for k in d)):
                raise ValueError(f"{name}: {what} is a dict whose keys are among {names!r}")
        if not isinstance(presence_col, (int, np.integer)) or presence_col >= widths[0][1]:
            raise ValueError(f"{name}: presence_col={presence_col!r} outside the history width {widths[0][1]} (< 0: everything counts)")
        if not max_workspace_mb > 0:
            raise ValueError(f"{name}: max_workspace_mb must be positive")
        return want, ents, srcs, widths

    def _knock_baseline(self, name, baseline, widths, dev):
        """``baseline`` (None, or a dict source name -> row [w]) as one contiguous fp32 row or None per source"""
        rows = []
        for k, wd in widths:
            row = None if baseline is None or baseline.get(k) is None else dev(baseline[k], th.float32).contiguous()
            if row is not None and row.shape != (wd,):
                raise ValueError(f"{name}: baseline[{k!r}] has shape {tuple(row.shape)}, the source's width is {wd}")
            rows.append(row)
        return rows

    @staticmethod
    def _knock_chunks(r, S, J, Ec, Jc, launch):
        """``launch(spec, es, js, first)`` -> its dict of [nA, En, S, ..] results, once per chunk of Ec whole environments (``es``, with the
        rows' ``spec`` cut to them) x Jc jobs (``js``; ``first``: the chunk that also asks for the base results), scattered into [nA,
        E, S, ..] tensors -- the per-pair ones, which have a job axis behind S, also along it.  One chunk: its dict as it is."""
        E, whole, res = r.E, Ec == r.E and Jc == J, {}
        for e0 in range(0, E, Ec):
            es = slice(e0, min(E, e0 + Ec))
            spec = r.spec
            if not whole:
                spec = ops.AcFeatureSpec(spec.N, [(t[es], wd, sn, sr) for t, wd, sn, sr in spec.sources], n_actions=spec.n_actions,
                                         last_action=None if spec.last_action is None else spec.last_action[es], la_strides=spec.la_strides,
                                         n_id=spec.n_id, T=S, T_phys=spec.T_phys)
            for j0 in range(0, J, Jc):
                js = slice(j0, min(J, j0 + Jc))
                part = launch(spec, es, js, j0 == 0)
                if whole:
                    return part
                for k, v in part.items():
                    pairwise = v.dim() >= 4 and k != "probs"
                    if k not in res:
                        shape = list(v.shape)
                        shape[1] = E
                        if pairwise:
                            shape[3] = J
                        res[k] = th.empty(shape, dtype=v.dtype, device=v.device)
                    if pairwise:
                        res[k][:, es, :, js] = v
                    else:
                        res[k][:, es] = v
        return res

    _KNOCK_RENAME = {"greedy_ko": "greedy", "greedy": "greedy_base", "shift_sq_actor": "state_shift_actor", "shift_sq_critic": "state_shift_critic",
                     "h_ko_actor": "h_actor_ko", "h_ko_critic": "h_critic_ko"}

    def _knock_results(self, out, res, want):
        """the launches' [nA, E, S, ..] results under the methods' names, environments first, into ``out``; the states only if wanted, the
        state shifts as distances; flip = a greedy action other than the base's"""
        for k, v in res.items():
            name = self._KNOCK_RENAME.get(k, k)
            if name in ("h_actor_ko", "h_critic_ko") and name not in want:
                continue
            v = v.permute(1, 2, 0, *range(3, v.dim()))
            out[name] = v.sqrt() if name.startswith("state_shift") else v
        if "greedy" in out:
            out["flip"] = out["greedy"] != out["greedy_base"].unsqueeze(-1)

    def _knock_presence(self, hist, ents, presence_col):
        """[E, S, nA, J] bool: the entity of job j is present in row (e, s, a) of ``hist`` [E, S, nA, N, d] (its ``presence_col`` != 0);
        always for job -1 and for ``presence_col`` < 0"""
        pres = th.as_tensor([j < 0 or presence_col < 0 for j in ents], device=self.device).expand(*hist.shape[:3], len(ents))
        if presence_col >= 0:
            idx = th.as_tensor([max(j, 0) for j in ents], device=self.device)
            pres = pres | (hist[..., presence_col].index_select(3, idx) != 0)
        return pres

    def _knock_means(self, out, cols, wt, per_env):
        """``out[name]`` = the mean of v with weight ``wt`` [E, S, nA, J] for every (name, v) of ``cols`` with a v, 0 where the weights
        sum to 0: float64 on the device, ``per_env`` taking a [E, S, nA, J] product to what one environment adds ([E, ..]), the
        environments added in their order"""
        cols = [(name, v) for name, v in cols if v is not None]
        parts = th.stack([per_env(v.to(th.float64) * wt) for _, v in cols] + [per_env(wt)])     # [n + 1, E, ..]: weighted sums | weights
        tot = th.zeros(parts.shape[0], *parts.shape[2:], dtype=th.float64, device=self.device)
        for e in range(parts.shape[1]):                                                           # environment order
            tot += parts[:, e]
        for k, (name, _) in enumerate(cols):
            out[name] = th.where(tot[-1] > 0, tot[k] / tot[-1].clamp_min(1e-300), th.zeros_like(tot[k]))

    KNOCKOUT_WANT = ("kl", "probs_ko", "logp_ko", "values_ko", "summary")

    def knockout(self, batch, entities=None, sources=None, baseline=None, override=None, target="recorded", which="both", hidden=None,
                 steps=None, want=("kl",), presence_col=0, max_workspace_mb=256):
        """Would this agent have acted differently, and would its critic have valued the state differently, if vehicle j had not been
        there?  The finite answer ``saliency`` cannot give (LayerNorm(F) rescales every other column when an entity's columns go, and the
        masked softmax flips near a tie): every row (e, s, agent) is run once per entity j of ``entities`` with j's columns of the selected
        ``sources`` replaced as the kernel gathers the features (ops.policy_knockout) -- the batch is read in place and not copied.
        ``batch``, ``target``, ``which``, ``hidden`` and ``steps`` as for ``saliency``: the GRU state of a row is the recorded one (or
        ``hidden``), given and held constant; nothing is carried through time.  With ``target="greedy"`` (or -1 entries) a* is the
        argmax of the row with NOTHING knocked, the same action for every j.
        ``entities``: entity indices in [0, N), None = all N; -1 = "nothing knocked" is allowed.  ``sources``: which of the names in
        ``_widths()`` are knocked, None = all.  ``baseline``: None (zeros) or a dict name -> row [w] that replaces the entity's columns.
        ``override``: a dict name -> tensor [E, S, nA, J, N, w] over the selected steps (any strides, innermost contiguous, read in
        place): job j of row (e, s, a) takes that source from override[e, s, a, j] instead of the batch; an overridden source is taken
        as given and not knocked as well.  This is how ``Prediction_policy.attention_knockout(..., want=("latent_ko",))`` continues into
        the policy.  The rollout writes ``attention_latent[:, t + 1] = GAT(history[:, t + 1], attention_latent[:, t], behavior_latent[:, t])``,
        so the ``latent_ko`` [E, S, nA, J, N, A] of ``attention_knockout(history[:, t0 + 1:t1 + 1], behavior_latent[:, t0:t1],
        attention_latent[:, t0:t1], want=("latent_ko",))`` is what ``attention_latent[:, t0 + 1:t1 + 1]`` would have held without entity j:
        ``knockout(batch, steps=slice(t0 + 1, t1 + 1), override={"attention_latent": latent_ko})`` with the same entity list closes
        "vehicle j unseen -> social context of every ego -> action and value" (INTEGRATION.md 1).
        Returns a dict; pair axes [E, S, nA, J]:
          kl = KL(pi_base || pi_ko), dlogp = logp_ko - logp_base (of a*), dvalue = V_ko - V_base, greedy (int64, lowest index on ties),
          flip = greedy != the base row's greedy;  base logp, values, target_action, greedy_base [E, S, nA] and probs [E, S, nA,
          n_actions];  knocked (the entity list), sources (the names that were knocked);
          probs_ko [.., n_actions], logp_ko, values_ko with those names in ``want``;
          entity_kl, entity_abs_dvalue, flip_rate [nA, J] float64 with "summary" in ``want``: means over the rows with weight
          ``batch["filled"]``, over the rows where the knocked entity is present (``history[..., j, presence_col] != 0``; every row
          for job -1, and for every job with ``presence_col`` < 0, as in ``attention_knockout``), 0 where no such row exists; formed on
          the device in float64, in environment order, from the per-pair outputs.
        ``want`` only ADDS results: kl, dlogp, dvalue, greedy and flip are always returned (and always counted in the chunk sizes), so
        the default ("kl",) and () ask for the same.
        Those of a net ``which`` leaves out are missing.  Rows and jobs are chunked so that one launch's outputs stay below
        ``max_workspace_mb``; chunked and unchunked calls give the same bits.  Where the replaced values equal the originals kl, dlogp
        and dvalue are exactly 0.  Unavailable actions have probability exactly 0 and contribute nothing to kl; a row with no
        available action is uniform (``policy_trace``'s convention) and has kl = 0.  Device tensors in -> device tensors out, numpy in
        -> numpy out.  Draws from no generator; parameters, gradient entries, optimiser state, ``hidden_states`` and the batch are not
        touched.  Not covered: layer_N / recurrent_N other than 1, knocking the GRU state; effects carried through time are ``knockout_trace``'s."""
        a = self.args
        want, ents, srcs, widths = self._knock_request("knockout", want, entities, sources, which, presence_col, max_workspace_mb,
                                                       baseline=baseline, override=override)
        nA, M, N = self.n_agents, a.rnn_hidden_dim, a.max_vehicle_num
        T1 = batch["history"].shape[1]
        one = isinstance(steps, (int, np.integer))
        if steps is None:
            t0, S = 0, T1
        elif one:
            t0, S = int(steps), 1
        else:
            t0, t1, stride = steps.indices(T1)
            if stride != 1 or t1 - t0 < 1:
                raise ValueError("knockout: steps is None, an int or a non-empty slice with step 1")
            S = t1 - t0
        r = self._rows(batch, t0, S)
        E, as_np, dev = r.E, r.as_np, r.dev
        J = len(ents)
        if hidden is None:
            ha, hc = r.field("rnn_states_actors", th.float32)[:, r.sl], r.field("rnn_states_critics", th.float32)[:, r.sl]
        else:
            ha, hc = (dev(h, th.float32) for h in hidden)
        assert ha.shape == hc.shape == (E, S, nA, M), (ha.shape, hc.shape, (E, S, nA, M))
        if ha.stride() != hc.stride() or ha.stride(3) != 1:
            ha, hc = ha.contiguous(), hc.contiguous()
        tgt, tgt_strides = self._target(r, target)
        w = {"actor": 0, "critic": 1, "both": 2}[which]
        base_rows, over = self._knock_baseline("knockout", baseline, widths, dev), []
        for k, wd in widths:
            ov = None if override is None or override.get(k) is None else dev(override[k], th.float32)
            if ov is not None:
                if ov.shape != (E, S, nA, J, N, wd):
                    raise ValueError(f"knockout: override[{k!r}] has shape {tuple(ov.shape)}, not {(E, S, nA, J, N, wd)}")
                if min(ov.stride()) < 0 or (wd > 1 and ov.stride(5) != 1):
                    ov = ov.contiguous()
            over.append(ov)
        knock = tuple(k in srcs for k, _ in widths)
        extra = tuple(k for k in ("probs_ko", "logp_ko", "values_ko") if k in want)
        ask = ("kl", "dlogp", "dvalue", "greedy_ko") + extra
        # chunks: whole environments x a range of jobs, one launch's per-pair outputs below the budget
        pair_bytes = nA * S * (4 * 3 + 8 + 4 * (("logp_ko" in extra) + ("values_ko" in extra) + a.n_actions * ("probs_ko" in extra)))
        budget = int(max_workspace_mb * 2 ** 20)
        Jc = max(1, min(J, budget // pair_bytes))
        Ec = max(1, min(E, budget // (pair_bytes * Jc)))

        def launch(spec, es, js, first):
            return ops.policy_knockout(self.actor_arena, self.critic_arena, w, spec, es.stop - es.start, S, nA, ents[js], h_actor=ha[es],
                                       h_critic=hc[es], h_strides=_esn(ha), avail=r.avail[es], avail_strides=_esn(r.avail),
                                       target=None if tgt is None else tgt[es], target_strides=tgt_strides, target_all=-1,
                                       n_actions=a.n_actions, knock=knock, baseline=base_rows,
                                       override=[None if ov is None else ov[es, :, :, js].permute(2, 0, 1, 3, 4, 5) for ov in over],
                                       want=ask + (("base",) if first else ()), packed=r.packed)

        out = {"knocked": tuple(ents), "sources": srcs}
        meta = tuple(out)
        self._knock_results(out, self._knock_chunks(r, S, J, Ec, Jc, launch), want)
        if "summary" in want:
            filled = dev(batch["filled"]).reshape(-1, T1)[:, r.sl].to(th.float64)                # [E, S]
            pres = self._knock_presence(r.field("history", th.float32)[:, r.sl], ents, presence_col)
            self._knock_means(out, (("entity_kl", out.get("kl")), ("entity_abs_dvalue", None if "dvalue" not in out else out["dvalue"].abs()),
                                    ("flip_rate", out.get("flip"))), filled[:, :, None, None] * pres, lambda x: x.sum(1))      # -> [nA, J]
        if one:
            keep = meta + ("entity_kl", "entity_abs_dvalue", "flip_rate")
            out = {k: (v if k in keep else v[:, 0]) for k, v in out.items()}
        return {k: (v if k in meta else v.cpu().numpy()) for k, v in out.items()} if as_np else out

    KNOCKOUT_TRACE_WANT = ("kl", "probs_ko", "logp_ko", "values_ko", "h_actor_ko", "h_critic_ko", "summary", "latent_shift")
    SOCIAL_KW = ("sources", "baseline", "noise", "deterministic", "tau", "hidden0")

    def knockout_trace(self, batch, entities=None, start=0, duration=1, horizon=None, sources=None, baseline=None, target="recorded",
                       which="both", hidden0=None, want=("kl",), presence_col=0, max_workspace_mb=256, override=None, override_base=None,
                       social=None, social_kw=None):
        """How long does the policy remember a vehicle?  Vehicle j is hidden from the agents for ``duration`` = D steps from step
        ``start`` and then shown again; the nets walk steps start .. start + H - 1 (``horizon`` = H, None: up to the batch's last
        step; ``duration`` None: knocked throughout, D = H) once per entity j of ``entities`` and once with nothing knocked, every
        chain with ITS OWN GRU state carried by the nets from a common start state (ops.policy_knockout_trace) -- what ``knockout``,
        whose state is given and held, leaves out.  In job j the inputs of steps start .. start + D - 1 have j's columns of the selected
        ``sources`` replaced as the kernel gathers the features (never the one-hots; the batch is read in place and not copied); steps
        start + D .. see the recorded inputs again, and the only trace of the knock there is the job's own state: the echo.
        ``batch``, ``entities`` (-1 = nothing knocked), ``sources``, ``baseline``, ``target``, ``which``, ``presence_col`` and
        ``max_workspace_mb`` as for ``knockout``; ``hidden0`` as for ``policy_trace``, taken at ``start``: None = the batch's
        ``rnn_states_*[:, start]``, "zeros", or a pair of [E, nA, M] tensors.  The last action is the recorded one, teacher-forced as in
        ``policy_trace``: the counterfactual does not re-decide past actions.  With ``target="greedy"`` a* is the BASE chain's argmax
        at that step, the same action for every job.
        Returns a dict; pair axes [E, H, nA, J]:
          kl = KL(pi_base || pi_ko), dlogp = logp_ko - logp_base (of a*), dvalue = V_ko - V_base, greedy (int64, lowest index on
          ties), flip = greedy != the base chain's greedy -- each against the base chain at the same step;
          state_shift_actor, state_shift_critic: the L2 distance of the job's GRU state from the base chain's after that step (the
          kernel's fp32 sum of squares in unit order, torch's sqrt);
          the base chain's logp, values, target_action, greedy_base [E, H, nA] and probs [E, H, nA, n_actions] (``policy_trace``'s bits);
          knocked (the entity list), sources (the names that were knocked), window = (start, D, H);
          probs_ko [.., n_actions], logp_ko, values_ko, h_actor_ko / h_critic_ko [.., M] (the job's state after every step) with those
          names in ``want``;
          echo_kl, echo_abs_dvalue, echo_flip_rate, echo_state_shift (of the actors; of the critics with which="critic") [nA, H, J]
          float64 with "summary" in ``want``: means over the environments with weight ``batch["filled"][:, start + h]``, over the
          pairs whose entity is present (``history[..., j, presence_col] != 0``) in at least one knocked step; every pair for job -1
          and for ``presence_col`` < 0; 0 where no such pair exists; formed on the device in float64, in environment order.
        ``want`` only ADDS results.  Those of a net ``which`` leaves out are missing.  Environments and jobs are chunked so that one
        launch's outputs and its per-step gate workspaces stay below ``max_workspace_mb``; chunked and unchunked calls give the same
        bits, and so do a shorter ``horizon`` (a prefix), packed or in-place fc1 and any ``want``.  A job whose replaced values equal
        the originals has kl = dlogp = dvalue = state_shift = 0.0 at every step.  Device tensors in -> device tensors out, numpy in ->
        numpy out.  Draws from no generator; parameters, gradient entries, optimiser state, ``hidden_states`` and the batch are not
        touched.
        ``override``: a dict name -> [E, H, nA, J, N, w] over the window (``knockout``'s rules: any strides, innermost contiguous, read
        in place): job j of step (e, h, a) takes that source from override[e, h, a, j] at EVERY step of the window, not only while
        h < D; an overridden source is taken as given and not knocked as well.  ``override_base``: a dict name -> [E, H, nA, N, w]: what
        the BASE chain (and a job -1 without an override of that source) reads instead of the batch's -- it needs an ``override``.
        With an override one ``iplan_ac_knockout_chain`` launch per chunk runs the knocked trunk over all H steps (the gate workspace
        is H deep and counted so) and the same walk; a job whose override rows equal ``override_base`` and whose knocked values equal
        the originals has kl = dlogp = dvalue = state_shift = 0.0 at every step.
        ``social``: a ``Prediction_policy`` -- the one-call chain "vehicle j out of sight for D steps -> the social context of every
        ego -> actions and values": per chunk of environments (and of jobs) ``social.attention_knockout_trace`` walks
        ``history[:, 1:]`` and ``behavior_latent[:, :-1]`` from ``attention_latent[:, start - 1]`` over the GAT window start - 1 ..
        start - 1 + H with the call's duration and entities; its ``latent_ko`` becomes override["attention_latent"] and its ``latent``
        (re-walked with nothing knocked, and with the same noise or none) the base override, so that the differences are the knock's
        alone; both are freed before the next chunk, the knocked latents never exist whole.  The alignment is the rollout's,
        ``attention_latent[:, t + 1] = GAT(history[:, t + 1], attention_latent[:, t], behavior_latent[:, t])``: GAT row start - 1 + h
        yields what policy step start + h reads.  It needs ``start >= 1``, ``GAT_enable``, entities in [0, N) and no explicit override
        of ``attention_latent``.  ``social_kw``: ``sources``, ``baseline``, ``noise`` ([nA, E, H, N, N-1, 2]), ``deterministic``,
        ``tau`` and ``hidden0`` ([E, nA, N, A]) of the GAT half, as ``attention_knockout_trace`` takes them.  The two halves' workspaces
        together stay below ``max_workspace_mb``.  With an override the result has ``overridden`` (the names), ``sources`` lists what
        was knocked in the policy (an overridden source is not among them), and with ``social`` and "latent_shift" in ``want`` the
        GAT's ``latent_shift`` [E, H, nA, N, J].
        Not covered: re-deciding the teacher-forced last action, knocking the GRU or GAT state itself, the forecast continuation,
        data-parallel aggregation, and layer_N / recurrent_N other than 1."""
        a = self.args
        want, ents, srcs, widths = self._knock_request("knockout_trace", want, entities, sources, which, presence_col, max_workspace_mb,
                                                       baseline=baseline, override=override, override_base=override_base)
        social_kw = {} if social_kw is None else social_kw
        if not isinstance(social_kw, dict) or any(k not in self.SOCIAL_KW for k in social_kw):
            raise ValueError(f"knockout_trace: social_kw is a dict whose keys are among {self.SOCIAL_KW}")
        if social is None and (social_kw or "latent_shift" in want):
            raise ValueError("knockout_trace: social_kw and want 'latent_shift' need social=")
        if social is not None:
            if not a.GAT_enable:
                raise ValueError("knockout_trace: social= needs GAT_enable: the policy reads no attention_latent")
            if not isinstance(start, (int, np.integer)) or start < 1:
                raise ValueError(f"knockout_trace: social= needs start >= 1 (got {start!r}): the GAT step before the window's first is walked")
            if any(d is not None and d.get("attention_latent") is not None for d in (override, override_base)):
                raise ValueError("knockout_trace: social= forms the override of attention_latent itself; an explicit one excludes it")
            if any(j < 0 for j in ents):
                raise ValueError("knockout_trace: social= takes entities in [0, N): the GAT half has no job -1")
        if isinstance(target, str) and target not in ("recorded", "greedy"):
            raise ValueError(f"knockout_trace: target={target!r}")
        nA, M = self.n_agents, a.rnn_hidden_dim
        T1 = batch["history"].shape[1]
        ints = (int, np.integer)
        if not isinstance(start, ints) or not 0 <= start < T1:
            raise ValueError(f"knockout_trace: start={start!r} outside [0, {T1})")
        start = int(start)
        H = T1 - start if horizon is None else horizon
        if not isinstance(H, ints) or not 1 <= H or start + H > T1:
            raise ValueError(f"knockout_trace: horizon={horizon!r} must satisfy 1 <= horizon and start + horizon <= {T1}")
        H = int(H)
        D = H if duration is None else duration
        if not isinstance(D, ints) or not 1 <= D <= H:
            raise ValueError(f"knockout_trace: duration={duration!r} outside [1, horizon={H}]")
        D = int(D)
        r = self._rows(batch, start, H)
        E, as_np, dev = r.E, r.as_np, r.dev
        J = len(ents)
        if isinstance(hidden0, str):
            if hidden0 != "zeros":
                raise ValueError(f"knockout_trace: hidden0={hidden0!r}")
            ha = hc = None
            hs = (0, 0)
        else:
            if hidden0 is None:
                ha, hc = r.field("rnn_states_actors", th.float32)[:, start], r.field("rnn_states_critics", th.float32)[:, start]
            else:
                ha, hc = (dev(h, th.float32) for h in hidden0)
            assert ha.shape == hc.shape == (E, nA, M), (ha.shape, hc.shape, (E, nA, M))
            if ha.stride() != hc.stride() or ha.stride(2) != 1:
                ha, hc = ha.contiguous(), hc.contiguous()
            hs = (ha.stride(1), ha.stride(0))
        if isinstance(target, str):
            tgt = r.acts if target == "recorded" else None
        else:
            t_in = dev(target, th.int64)
            assert t_in.shape == r.acts.shape, (t_in.shape, tuple(r.acts.shape))
            full = th.full((E, T1, nA), -1, dtype=th.int64, device=self.device)    # (addressed by physical row, like the batch's fields)
            full[:, r.sl] = t_in
            tgt = full[:, r.sl]
        base_rows = self._knock_baseline("knockout_trace", baseline, widths, dev)
        N = a.max_vehicle_num
        over, over_base = [], []
        for dst, given, shape, what in ((over, override, (E, H, nA, J, N), "override"), (over_base, override_base, (E, H, nA, N), "override_base")):
            for k, wd in widths:
                ov = None if given is None or given.get(k) is None else dev(given[k], th.float32)
                if ov is not None:
                    if ov.shape != shape + (wd,):
                        raise ValueError(f"knockout_trace: {what}[{k!r}] has shape {tuple(ov.shape)}, not {shape + (wd,)}")
                    if min(ov.stride()) < 0 or (wd > 1 and ov.stride(-1) != 1):
                        ov = ov.contiguous()
                dst.append(ov)
        overridden = tuple(k for (k, _), ov in zip(widths, over) if ov is not None or (social is not None and k == "attention_latent"))
        if not overridden and any(ov is not None for ov in over_base):
            raise ValueError("knockout_trace: override_base needs an override: without one the base chain is the batch's")
        srcs = tuple(k for k in srcs if k not in overridden)
        knock = tuple(k in srcs for k, _ in widths)
        w = {"actor": 0, "critic": 1, "both": 2}[which]
        extra = tuple(k for k in ("probs_ko", "logp_ko", "values_ko") if k in want)
        want_h = tuple(k for k in ("h_actor_ko", "h_critic_ko") if k in want)
        ask = ("kl", "dlogp", "dvalue", "greedy_ko", "shift_sq") + extra + (("h_ko",) if want_h else ())
        # chunks: whole environments x a range of jobs; one launch's per-pair outputs and gate workspaces below the budget
        GI = 4 * ops.L.AC_TRACE_GI
        pair_bytes = nA * H * (4 * 5 + 8 + 4 * (("logp_ko" in extra) + ("values_ko" in extra) + a.n_actions * ("probs_ko" in extra)) + 8 * M * bool(want_h))
        job_bytes = pair_bytes + 2 * nA * (H if overridden else D) * GI * 16 // 15 + 1         # (an override: the trunk covers all H steps
        env_bytes = 0 if overridden else 2 * nA * H * GI                                       #  and there is no base gi)
        gat_env = gat_job = 0
        if social is not None:
            # the GAT half of a chunk, as attention_knockout_trace counts it: the noise and the base walk's latents per environment,
            # latent_ko (and the shifts) per (environment, job)
            A, g_shift = a.attention_dim, "latent_shift" in want
            gat_env = 4 * nA * H * (2 * N * (N - 1) + N * A)
            gat_job = 4 * nA * H * (N * A + (N if g_shift else 0))
            g_hist = r.field("history", th.float32)[:, 1:]
            g_beh = r.field("behavior_latent", th.float32)[:, :-1] if social.args.GAT_use_behavior else None
            g_h0 = social_kw.get("hidden0")
            g_h0 = r.field("attention_latent", th.float32)[:, start - 1] if g_h0 is None else dev(g_h0, th.float32)
            g_noise = social_kw.get("noise")
            g_noise = None if g_noise is None else dev(g_noise, th.float32)
            g_kw = {k: social_kw[k] for k in ("sources", "baseline", "deterministic", "tau") if k in social_kw}
            ia = [k for k, _ in widths].index("attention_latent")
        env_bytes += gat_env
        job_bytes += gat_job
        budget = int(max_workspace_mb * 2 ** 20)
        Jc = max(1, min(J, (budget - env_bytes) // job_bytes))
        if Jc < J and Jc > 15:
            Jc -= Jc % 15                                                                      # whole tiles
        Ec = max(1, min(E, budget // (env_bytes + job_bytes * Jc)))

        def launch(spec, es, js, first):
            ovs = [None if ov is None else ov[es, :, :, js].permute(2, 0, 1, 3, 4, 5) for ov in over]
            ovb = [None if ov is None else ov[es].permute(2, 0, 1, 3, 4) for ov in over_base]
            g = None
            if social is not None:
                En, Jn = es.stop - es.start, len(ents[js])
                g = social.attention_knockout_trace(g_hist[es], None if g_beh is None else g_beh[es], hidden0=g_h0[es], entities=ents[js],
                                                    start=start - 1, duration=D, horizon=H, noise=None if g_noise is None else g_noise[:, es],
                                                    want=("latent_ko",) + (("shift",) if g_shift else ()), presence_col=presence_col,
                                                    max_workspace_mb=En * (gat_env + Jn * gat_job) / 2 ** 20, **g_kw)
                ovs[ia], ovb[ia] = g["latent_ko"].permute(2, 0, 1, 3, 4, 5), g["latent"].permute(2, 0, 1, 3, 4)
            part = ops.policy_knockout_trace(self.actor_arena, self.critic_arena, w, spec, es.stop - es.start, H, D, nA, ents[js],
                                             hidden0_actor=None if ha is None else ha[es], hidden0_critic=None if hc is None else hc[es],
                                             h_strides=hs, avail=r.avail[es], avail_strides=(r.avail.stride(2), r.avail.stride(1)),
                                             target=None if tgt is None else tgt[es],
                                             target_strides=(0, 0) if tgt is None else (tgt.stride(2), tgt.stride(1)),
                                             n_actions=a.n_actions, knock=knock, baseline=base_rows,
                                             want=ask + (("base",) if first else ()), packed=r.packed, override=ovs, override_base=ovb)
            if g is not None and g_shift:
                part["latent_shift"] = g["latent_shift"].permute(2, 0, 1, 4, 3).contiguous()    # [nA, En, H, Jn, N]: scattered as a pair tensor
            del g, ovs, ovb                                                                     # (freed before the next chunk)
            return part

        out = {"knocked": tuple(ents), "sources": srcs, "window": (start, D, H)}
        if overridden:
            out["overridden"] = overridden
        meta = tuple(out)
        self._knock_results(out, self._knock_chunks(r, H, J, Ec, Jc, launch), want)
        if "latent_shift" in out:
            out["latent_shift"] = out["latent_shift"].transpose(3, 4)                            # [E, H, nA, N, J], the GAT method's axes
        if "summary" in want:
            filled = dev(batch["filled"]).reshape(-1, T1)[:, r.sl].to(th.float64)                # [E, H]
            pres = self._knock_presence(r.field("history", th.float32)[:, start:start + D], ents, presence_col).any(1)   # in a knocked step
            shift = out.get("state_shift_actor", out.get("state_shift_critic"))
            self._knock_means(out, (("echo_kl", out.get("kl")), ("echo_abs_dvalue", None if "dvalue" not in out else out["dvalue"].abs()),
                                    ("echo_flip_rate", out.get("flip")), ("echo_state_shift", shift)),
                              filled[:, :, None, None] * pres[:, None], lambda x: x.permute(0, 2, 1, 3))                      # -> [nA, H, J]
        return {k: (v if k in meta else v.cpu().numpy()) for k, v in out.items()} if as_np else out

    def get_value_ippo(self, agent_id, obs, rnn_states_critic):
        """controllers/dcntrl_controller.py:61-68."""
        obs_in = obs.reshape(-1, 1, obs.shape[-1])
        hidden_in = rnn_states_critic.reshape(self.args.recurrent_N, -1, self.args.rnn_hidden_dim)
        value, _ = self.critics[agent_id](obs_in, hidden_in)
        return value.reshape(*obs.shape[:-1], 1)

    def eval_action_ippo(self, agent_id, obs, action, available_actions, rnn_states_actor):
        """controllers/dcntrl_controller.py:70-85."""
        obs_in = obs.reshape(-1, 1, obs.shape[-1])
        hidden_in = rnn_states_actor.reshape(self.args.recurrent_N, -1, self.args.rnn_hidden_dim)
        action_in = action.reshape(-1, 1, 1)
        avail_in = available_actions.reshape(-1, 1, available_actions.shape[-1])
        logp, ent = self.agents[agent_id].evaluate_actions(obs_in, hidden_in, action_in, avail_in)
        return logp.reshape(*obs.shape[:-1], 1), ent

    def _build_inputs_ippo(self, agent_id, batch, action_onehot, discr_signal=None):
        """Assembled [bs, T, F] tensor for callers that want it (dcntrl_controller.py:87-115);
        pure concatenation, no arithmetic.  The fused learner path does not use it."""
        bs, num_ts = batch["history"].shape[:2]
        states = [batch["history"]]
        if self.args.GAT_enable:
            states.append(batch["attention_latent"])
        if self.args.Behavior_enable:
            states.append(batch["behavior_latent"])
        inputs = [th.cat(states, dim=-1).reshape(bs, num_ts, -1)]
        if self.args.obs_last_action:
            inputs.append(th.cat([action_onehot[:, 0].unsqueeze(1), action_onehot[:, :-1]], dim=1))
        if self.args.obs_agent_id:
            onehot = th.zeros((bs, num_ts, self.n_agents), device=inputs[0].device)
            onehot[:, :, agent_id] = 1
            inputs.append(onehot)
        return th.cat(inputs, dim=-1)

    def _build_inputs(self, batch, t):
        """dcntrl_controller.py:187-213 (assembled [bs, nA, F]; tensor plumbing only)."""
        bs = batch.batch_size
        states = [batch["history"][:, t]]
        if self.args.GAT_enable:
            states.append(batch["attention_latent"][:, t])
        if self.args.Behavior_enable:
            states.append(batch["behavior_latent"][:, t])
        inputs = [th.cat(states, dim=-1)]
        if self.args.obs_last_action:
            inputs.append(th.zeros_like(batch["actions_onehot"][:, t]) if t == 0 else batch["actions_onehot"][:, t - 1])
        if self.args.obs_agent_id:
            inputs.append(th.eye(self.n_agents, device=inputs[0].device).unsqueeze(0).expand(bs, -1, -1))
        return th.cat([x.reshape(bs, self.n_agents, -1) for x in inputs], dim=2)

    # ------------------------------------------------------------------------------ bookkeeping
    def init_hidden(self, batch_size):
        self.hidden_states = None

    def parameters(self):
        return [list(agent.parameters()) for agent in self.agents]

    def critic_parameters(self):
        return [list(critic.parameters()) for critic in self.critics]

    def load_state(self, other_mac):
        for i, agent in enumerate(self.agents):
            agent.load_state_dict(other_mac.agents[i].state_dict())

    def cuda(self):
        pass                                  # arenas are created on args.device already

    def set_train_mode(self):
        for m in self.agents + self.critics:
            m.train()

    def set_eval_mode(self):
        for m in self.agents + self.critics:
            m.eval()

    def save_models(self, path):
        for i, agent in enumerate(self.agents):
            th.save(agent.state_dict(), f"{path}/agent_{i}.th")
        for i, critic in enumerate(self.critics):
            th.save(critic.state_dict(), f"{path}/critic_{i}.th")

    def load_models(self, paths):
        if len(paths) == 1:
            paths = [copy.copy(paths[0]) for _ in range(self.n_agents)]
        for i, agent in enumerate(self.agents):
            agent.load_state_dict(th.load(f"{paths[i]}/agent_{i}.th", map_location="cpu"))
        for i, critic in enumerate(self.critics):
            critic.load_state_dict(th.load(f"{paths[i]}/critic_{i}.th", map_location="cpu"))

    def _build_agents(self, input_shape):
        self.agents = [R_Actor(input_shape, self.args) for _ in range(self.n_agents)]

    def _build_critics(self, input_shape):
        self.critics = []
        if self.args.critic is not None:
            self.critics = [R_Critic(input_shape, self.args) for _ in range(self.n_agents)]

    def _get_input_shape(self, scheme):
        h = scheme["history"]["vshape"]
        shape = h[0] * h[1]
        if self.args.GAT_enable:
            s = scheme["attention_latent"]["vshape"]
            shape += s[0] * s[1]
        if self.args.Behavior_enable:
            s = scheme["behavior_latent"]["vshape"]
            shape += s[0] * s[1]
        if self.args.obs_last_action:
            shape += scheme["actions_onehot"]["vshape"][0]
        if self.args.obs_agent_id:
            shape += self.n_agents
        return shape
