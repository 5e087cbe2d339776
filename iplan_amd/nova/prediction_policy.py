"""Prediction_policy -- instant-incentive inference module (mirror of nova/prediction_policy.py:14-286).

Owns n_agents x (GAT_Net, Prediction_Decoder) with one optimiser per agent, exactly like the
reference, but the weights of all agents live in two stacked arenas so that
``GAT_latent_update`` is ONE fused launch over (agent, env) and ``learn`` is one forward and one
backward launch sequence for all agents.
"""
import copy

import numpy as np
import torch

from .. import ops
from ..arena import ParamArena
from ..optim import FusedAdam, step_all
from ..streams import AsyncHost
from .GAT_Net import GAT_Net, gumbel_noise
from .prediction_net import Prediction_Decoder

EPS = 1e-10


def _as_dev(x, device):
    """numpy / tensor -> fp32 tensor on device (the runner hands float64 numpy arrays over)."""
    if isinstance(x, np.ndarray):
        return torch.as_tensor(x, dtype=torch.float32).to(device)
    return x.to(device=device, dtype=torch.float32)


def _halving_sum(x, dim):
    """sum over ``dim`` in a fixed order any host can restate: the axis is zero-padded to a power of two, then its upper half is
    added to its lower half, elementwise, until one entry is left"""
    n = x.shape[dim]
    size = 1
    while size < n:
        size *= 2
    if size > n:
        pad = list(x.shape)
        pad[dim] = size - n
        x = torch.cat([x, torch.zeros(pad, dtype=x.dtype, device=x.device)], dim=dim)
    while size > 1:
        size //= 2
        x = x.narrow(dim, 0, size) + x.narrow(dim, size, size)
    return x.squeeze(dim)


class Prediction_policy:
    def __init__(self, args, logger):
        self.device = torch.device("cuda" if args.use_cuda else "cpu")
        self.args = args
        self.n_actions = args.n_actions
        self.n_agents = args.n_agents
        self.max_vehicle_num = args.max_vehicle_num
        self.max_history_len = args.max_history_len
        self.max_episode_len = args.episode_limit
        self.prediction_batch_size = args.pred_batch_size
        self.pred_length = args.pred_length
        self.optim_eps = args.optim_eps
        self.weight_decay = args.weight_decay
        self.obs_shape = args.obs_shape_single
        self.logger = logger
        self.log_prefix = args.log_prefix
        self.log_stats_t = -self.args.learner_log_interval - 1
        self.GAT_input_dim = args.obs_shape_single + (args.latent_dim if args.GAT_use_behavior else 0)
        self.init_GAT_net()
        self._use_max_grad_norm = args.use_max_grad_norm
        self.max_grad_norm = args.max_grad_norm

    def init_GAT_net(self):
        """nova/prediction_policy.py:64-88 (same construction order -> same seeded init)."""
        a = self.args
        self.pred_GAT, self.pred_decoder = [], []
        for _ in range(self.n_agents):
            self.pred_GAT.append(GAT_Net(input_shape=self.GAT_input_dim, args=a))
            self.pred_decoder.append(Prediction_Decoder(
                input_size=a.obs_shape_single, hidden_size=a.attention_dim, output_size=a.obs_shape_single,
                num_layers=1, pred_length=a.pred_length, teacher_forcing_ratio=a.teacher_forcing_ratio,
                dropout=a.decoder_dropout))
        self.gat_arena = ParamArena(self.pred_GAT, self.device)
        self.dec_arena = ParamArena(self.pred_decoder, self.device)
        ParamArena.colocate_grads([self.gat_arena, self.dec_arena])      # one gradient collective per learn() instead of two
        for i in range(self.n_agents):
            self.pred_GAT[i].attach(self.gat_arena, i)
            self.pred_decoder[i].attach(self.dec_arena, i)
        self.pred_optimizer = [
            FusedAdam([(self.gat_arena, i), (self.dec_arena, i)], lr=a.lr_predict, eps=self.optim_eps,
                      weight_decay=self.weight_decay) for i in range(self.n_agents)]

    # ---------------------------------------------------------------------------- rollout
    def GAT_latent_update(self, history_single, encoder_hidden, behavior_latent=None, noise=None, out=None, fuse_enc=None, fuse_ac=None):
        """history_single [E,nA,N,d], encoder_hidden [E,nA,N,A], behavior_latent [E,nA,N,Z] ->
        attention latent [E,nA,N,A]  (nova/prediction_policy.py:92-118).
        numpy in -> numpy out (drop-in for ParallelRunner); device tensors in -> device tensor out.
        ``noise``: pre-drawn gumbel samples [nA,E,N,N-1,2]; ``out``: optional [E,nA,N,A] destination view
        (e.g. ``batch["attention_latent"][:, t + 1]``) the kernel writes in place."""
        as_np = isinstance(history_single, np.ndarray)
        hist = _as_dev(history_single, self.device)
        hid = _as_dev(encoder_hidden, self.device)
        E, nA, N, _ = hist.shape
        lat = None
        if self.args.GAT_use_behavior:
            lat = _as_dev(behavior_latent, self.device).permute(1, 0, 2, 3)
        if noise is None:
            noise = gumbel_noise((nA, E, N, N - 1, 2), self.device)
        out, _ = ops.gat_forward(self.gat_arena, hist.permute(1, 0, 2, 3), lat, hid.permute(1, 0, 2, 3), noise,
                                 out=None if out is None else out.permute(1, 0, 2, 3), fuse_enc=fuse_enc, fuse_ac=fuse_ac)
        out = out.permute(1, 0, 2, 3)          # [E, nA, N, A] view
        return out.cpu().numpy() if as_np else out

    # ---------------------------------------------------------------------------- inference
    def _beh_latent(self, who, behavior_latent, shape=None):
        """the behaviour latent the GAT of ``who``'s call reads, fp32 on the device in the caller's layout (of ``shape``, where one is
        given); None where this policy's GAT reads none"""
        if not self.args.GAT_use_behavior:
            return None
        if behavior_latent is None:
            raise ValueError(f"{who}: this policy's GAT reads the behaviour latent (GAT_use_behavior), behavior_latent is needed")
        lat = _as_dev(behavior_latent, self.device)
        if shape is not None and lat.shape != shape:
            raise ValueError(f"{who}: behavior_latent {tuple(lat.shape)} != {shape}")
        return lat

    def _noise(self, noise, deterministic, nA, b0, b1, inner, zeros=True):
        """the gumbel samples [nA, b1 - b0, *inner] of rows b0 .. b1 - 1: that slice of a given ``noise``, else a draw from torch's
        generator; ``deterministic``: no noise -- zeros (l + 0 is exact: the gate of no noise), or None where the kernel takes that"""
        if deterministic:
            return torch.zeros(nA, b1 - b0, *inner, dtype=torch.float32, device=self.device) if zeros else None
        if noise is not None:
            return noise[:, b0:b1].to(device=self.device, dtype=torch.float32).contiguous()
        return gumbel_noise((nA, b1 - b0, *inner), self.device)

    def _start_offsets(self, hist):
        """int64 [nA, E] on the device: the element offset of (env, agent, entity 0, feature 0) from the first element of ``hist``
        [E, nA, N, d]; every row these offsets lead a kernel to lies inside hist's storage (checked here, on the host)"""
        E, nA, N, d = hist.shape
        offset = (torch.arange(nA)[:, None] * hist.stride(1) + torch.arange(E)[None, :] * hist.stride(0)).to(torch.int64)
        assert int(offset.max()) + (N - 1) * hist.stride(2) + d <= ops._room(hist)
        return offset.to(self.device)

    def predict(self, history_single, attention_hidden, behavior_latent=None, noise=None):
        """Where will the entities be in the next ``pred_length`` steps?  history_single [E,nA,N,d], attention_hidden
        [E,nA,N,A], behavior_latent [E,nA,N,Z] -> predicted states [E,nA,N,P,d]: one GAT forward and one decoder launch for
        all agents, the decoder as ``Prediction_Decoder.forward(last_state, None, hidden)`` runs it under ``.eval()``
        (nova/prediction_net.py:40-63: autoregressive, no teacher forcing, no dropout).  numpy in -> numpy out; device
        tensors in -> device tensor out.  ``noise``: pre-drawn gumbel samples [nA,E,N,N-1,2]."""
        as_np = isinstance(history_single, np.ndarray)
        hist = _as_dev(history_single, self.device)
        hid = _as_dev(attention_hidden, self.device)
        E, nA, N, d = hist.shape
        if hist.stride(3) != 1:
            hist = hist.contiguous()
        lat = None
        if self.args.GAT_use_behavior:
            lat = _as_dev(behavior_latent, self.device).permute(1, 0, 2, 3)
        if noise is None:
            noise = gumbel_noise((nA, E, N, N - 1, 2), self.device)
        h0, _ = ops.gat_forward(self.gat_arena, hist.permute(1, 0, 2, 3), lat, hid.permute(1, 0, 2, 3), noise)
        out = ops.predict(self.dec_arena, hist, self._start_offsets(hist), hist.stride(2), 0, h0.reshape(nA, E * N, -1), N,
                          self.pred_length, d, checked=True)
        pred = out["pred"].view(nA, E, N, self.pred_length, d).permute(1, 0, 2, 3, 4)
        return pred.cpu().numpy() if as_np else pred

    def evaluate(self, batch, stride=1, pos=(1, 2), presence_col=0, noise=None, max_samples_per_launch=512, defer=False):
        """Displacement error of the predictor over an episode batch, dense: every start step t = 0, stride, ... < T - P - 1
        (T as ``learn`` defines it) of every episode, for all agents.  A sample counts when that agent's ``terminated`` flag
        is clear at t ... t + P (and ``filled``, where the batch carries it, is set there); a row (entity) counts at horizon
        step p when its presence column is non-zero at t and at t + p + 1.  ``pos``: the position columns, ``presence_col``:
        the presence column (< 0: every row counts) -- the defaults are highway's layout after the wrapper strips the id
        (presence, x, y, vx, vy).  The samples go through the GAT and the decoder in chunks of ``max_samples_per_launch``
        (the gumbel tensor alone is 119 KB per sample at 55 entities and 5 agents); targets are read in place from the
        history field, nothing but the three metric sums per (agent, step) is written, and the chunks' sums are added in chunk
        order.  ``noise``: pre-drawn gumbel samples [nA, E * n_starts, N, N-1, 2] in (episode, start) order; drawn from
        torch's generator otherwise.  Returns a dict of host arrays after ONE read-back: ``displacement`` [nA, P] (mean
        ||pos error|| per horizon step), ``ade`` [nA] (mean over steps and rows), ``fde`` [nA] (last step), ``l1`` [nA, P] (mean
        per row of the summed absolute error over all columns), ``count`` [nA, P] (summed weights); a horizon nothing counts
        for reports NaN.  ``defer=True``: everything is enqueued and a ``finish()`` callable is returned.  Parameters and
        optimiser state are not touched."""
        a, dev = self.args, self.device
        nA, N, P = self.n_agents, self.max_vehicle_num, self.pred_length
        history = batch["history"][:, :-1].to(device=dev, dtype=torch.float32)
        attention = batch["attention_latent"][:, :-1].to(device=dev, dtype=torch.float32)
        latent = batch["behavior_latent"][:, :-1].to(device=dev, dtype=torch.float32) if a.GAT_use_behavior else None
        ok = batch["terminated"][:, :-1].to(dev)[..., 0] == 0                     # [E, T, nA]
        try:
            filled = batch["filled"]
        except (KeyError, ValueError):
            filled = None
        if filled is not None:
            ok = ok & (filled[:, :-1].to(dev).reshape(ok.shape[0], ok.shape[1], 1) != 0)
        E, T = history.shape[:2]
        d = history.shape[-1]
        avail_len = T - P - 1
        assert avail_len >= 1 and stride >= 1 and max_samples_per_launch >= 1, (T, P, stride)
        assert history.stride(4) == 1
        starts = torch.arange(0, avail_len, stride)
        n_t = starts.numel()
        S_all = E * n_t
        ei = torch.arange(E).repeat_interleave(n_t)                               # sample = (episode, start), episode-major
        ti = starts.repeat(E)
        # element offset of (e, t, agent, entity 0, feature 0) in the history view, per (agent, sample): host arithmetic, so
        # the bound on what the kernel will read is checked here, without a read-back
        sE, sT, sA, sN, _ = history.stride()
        offset = (torch.arange(nA)[:, None] * sA + (ei * sE + ti * sT)[None, :]).to(torch.int64)
        assert int(offset.max()) + (N - 1) * sN + P * sT + d <= ops._room(history)
        offset = offset.to(dev)
        ei, ti = ei.to(dev), ti.to(dev)
        weight = ok.unfold(1, P + 1, 1).all(-1)[ei, ti].to(torch.float32).t().contiguous()      # [nA, S_all]
        if noise is not None:
            assert noise.shape == (nA, S_all, N, N - 1, 2), (noise.shape, (nA, S_all, N, N - 1, 2))
        total = torch.zeros(nA, P, 3, dtype=torch.float32, device=dev)
        for c0 in range(0, S_all, max_samples_per_launch):
            c1 = min(S_all, c0 + max_samples_per_launch)
            e_c, t_c = ei[c0:c1], ti[c0:c1]
            x0 = history[e_c, t_c].permute(1, 0, 2, 3)                            # the GAT's inputs are gathered (data movement only)
            att = attention[e_c, t_c].permute(1, 0, 2, 3)
            lat = latent[e_c, t_c].permute(1, 0, 2, 3) if latent is not None else None
            nz = noise[:, c0:c1].contiguous().to(dev) if noise is not None else gumbel_noise((nA, c1 - c0, N, N - 1, 2), dev)
            h0, _ = ops.gat_forward(self.gat_arena, x0, lat, att, nz)
            out = ops.predict(self.dec_arena, history, offset[:, c0:c1].contiguous(), sN, sT, h0.reshape(nA, (c1 - c0) * N, -1), N, P, d,
                              want_pred=False, want_metrics=True, weight=weight[:, c0:c1].contiguous(), presence_col=presence_col,
                              pos=pos, checked=True)
            total += out["metrics"]
        staged = AsyncHost(total) if defer else None

        def finish():
            m = (staged.get() if staged is not None else total.cpu()).numpy().astype(np.float64)      # ONE host read-back
            count = m[..., 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                disp = np.where(count > 0, m[..., 0] / count, np.nan)
                l1 = np.where(count > 0, m[..., 1] / count, np.nan)
                ade = np.where(count.sum(1) > 0, m[..., 0].sum(1) / count.sum(1), np.nan)
            return {"displacement": disp, "ade": ade, "fde": disp[:, -1].copy(), "l1": l1, "count": count}
        return finish if defer else finish()

    # ---------------------------------------------------------------------------- attention inspection
    def attention_map(self, history_single, attention_hidden, behavior_latent=None, noise=None, deterministic=False, presence_col=0):
        """Which neighbours does each agent's GAT attend to at ONE step?  history_single [E,nA,N,d], attention_hidden [E,nA,N,A],
        behavior_latent [E,nA,N,Z] (ignored without ``GAT_use_behavior``) -> dict of ``attention``, ``soft``, ``hard`` [E,nA,N,N]
        and ``latent`` [E,nA,N,A].  The maps are indexed by ENTITY: ``[e, a, i, j]`` is what ego i gives entity j -- ``soft`` the
        softmax weight, ``hard`` the gumbel-softmax gate, ``attention`` their product (the weight the value of j enters the
        aggregate of i with); the diagonal is 0.  ``latent`` is bit-for-bit what ``GAT_latent_update`` returns for the same
        inputs and noise.  ``noise``: pre-drawn gumbel samples [nA,E,N,N-1,2], drawn from torch's generator when None;
        ``deterministic=True`` uses no noise at all (the gate is sigmoid((l1 - l0) / tau)) and draws nothing.  numpy in -> numpy
        out, device tensors in -> device tensors out.  One launch (``attention_trace``'s kernel with one step); parameters,
        gradients and optimiser state are not touched."""
        as_np = isinstance(history_single, np.ndarray)
        hist = _as_dev(history_single, self.device).unsqueeze(1)
        hid = _as_dev(attention_hidden, self.device)
        lat = self._beh_latent("attention_map", behavior_latent)
        lat = None if lat is None else lat.unsqueeze(1)
        if noise is not None and not deterministic:
            noise = _as_dev(noise, self.device).unsqueeze(2)
        res = self.attention_trace(hist, lat, hidden0=hid, noise=noise, deterministic=deterministic, want=("attention", "soft", "hard"),
                                   presence_col=presence_col, max_envs_per_launch=hist.shape[0], _stats=False)
        out = {k: res[k][:, 0] for k in ("attention", "soft", "hard", "latent")}
        return {k: v.cpu().numpy() for k, v in out.items()} if as_np else out

    def attention_trace(self, history, behavior_latent=None, hidden0=None, noise=None, deterministic=False, want=("attention",),
                        weight=None, presence_col=0, max_envs_per_launch=64, defer=False, _stats=True):
        """How does the attention evolve over an episode?  Walks the GAT over the S steps of ``history`` [E,S,nA,N,d] (with
        ``behavior_latent`` [E,S,nA,N,Z]; ignored without ``GAT_use_behavior``) from ``hidden0`` [E,nA,N,A] (None: zeros) in one
        launch per chunk of environments: latent_s = GAT(history_s, behavior_latent_s, latent_{s-1}).  Returns a dict with
        ``latent`` [E,S,nA,N,A], the maps named in ``want`` (any of ``attention``, ``soft``, ``hard``: [E,S,nA,N,N], indexed by
        entity as ``attention_map`` describes) and ``stats``, host arrays [nA,S] after ONE read-back:
          ``gate``               mean gumbel gate over the (ego, neighbour) pairs with both present
          ``attention_per_ego``  attention mass (soft * hard over those pairs) per present ego
          ``present_mass``       softmax mass a present ego gives present neighbours (the rest went to empty slots)
          ``entropy``            entropy of a present ego's softmax over its N-1 neighbours
          ``egos``, ``pairs``    the weighted counts the means are taken over; a step nothing counts at reports NaN.
        An entity is present when column ``presence_col`` of its history row is non-zero (< 0: every entity counts); ``weight``
        [E,S,nA] (e.g. ``1 - terminated`` times ``filled``) weighs every (env, step, agent), None = 1.  The sums over the
        environments are taken in float64 in environment order, so they do not depend on ``max_envs_per_launch`` (the chunk
        size: the gumbel tensor is N (N-1) 2 S floats per scene).  ``noise``: pre-drawn gumbel samples [nA,E,S,N,N-1,2]; None
        draws them from torch's generator as ``GAT_latent_update`` does; ``deterministic=True`` passes no noise and draws
        nothing.  numpy in -> numpy out, device tensors in -> device tensors out.  ``defer=True``: everything is enqueued and a
        ``finish()`` callable returning the dict is handed back.  Parameters, gradients and optimiser state are not touched.

        Replaying a rollout (the alignment of ``SyntheticLoop``'s rollout: step t reads the history of t + 1 and the latents of
        t): with ``b = batch`` and the per-step noise the rollout used, stacked as [nA,E,T,N,N-1,2],
            ``attention_trace(b["history"][:, 1:], b["behavior_latent"][:, :-1], hidden0=b["attention_latent"][:, 0], noise=...)``
        gives ``latent == b["attention_latent"][:, 1:]`` bit for bit."""
        as_np = isinstance(history, np.ndarray)
        dev = self.device
        hist = _as_dev(history, dev)
        E, S, nA, N, d = hist.shape
        A = self.args.attention_dim
        assert max_envs_per_launch >= 1
        want = tuple(want)
        names = {"attention": "attn", "soft": "soft", "hard": "hard"}
        assert all(k in names for k in want), want
        if hist.stride(4) != 1 or hist.stride(3) != d:
            hist = hist.contiguous()
        lat = self._beh_latent("attention_trace", behavior_latent)
        if lat is not None:
            if lat.stride(4) != 1 or lat.stride(3) != lat.shape[4]:
                lat = lat.contiguous()
            lat = lat.permute(2, 0, 1, 3, 4)
        src0 = hist.permute(2, 0, 1, 3, 4)                                        # [nA, E, S, N, d] view, read in place
        h0 = None
        if hidden0 is not None:
            h0 = _as_dev(hidden0, dev)
            if h0.stride(3) != 1 or h0.stride(2) != A or h0.data_ptr() % 16 or h0.stride(0) % 4 or h0.stride(1) % 4:
                h0 = h0.contiguous()
            h0 = h0.permute(1, 0, 2, 3)
        if deterministic:
            noise = None
        elif noise is not None:
            noise = _as_dev(noise, dev)
            assert noise.shape == (nA, E, S, N, N - 1, 2), (noise.shape, (nA, E, S, N, N - 1, 2))
        w = None
        if weight is not None:
            w = _as_dev(weight, dev)
            assert w.shape == (E, S, nA), w.shape
            w = w.permute(2, 0, 1)
        res = {"latent": torch.empty(E, S, nA, N, A, dtype=torch.float32, device=dev)}
        for k in want:
            res[k] = torch.empty(E, S, nA, N, N, dtype=torch.float32, device=dev)
        parts = []
        for e0 in range(0, E, max_envs_per_launch):
            e1 = min(E, e0 + max_envs_per_launch)
            nz = self._noise(noise, deterministic, nA, e0, e1, (S, N, N - 1, 2), zeros=False)
            out = {"latent": res["latent"][e0:e1].permute(2, 0, 1, 3, 4)}
            for k in want:
                out[names[k]] = res[k][e0:e1].permute(2, 0, 1, 3, 4)
            got = ops.gat_trace(self.gat_arena, src0[:, e0:e1], None if lat is None else lat[:, e0:e1], None if h0 is None else h0[:, e0:e1],
                                nz, want=tuple(out) + (("stats",) if _stats else ()), weight=None if w is None else w[:, e0:e1].contiguous(),
                                presence_col=presence_col, out=out)
            if _stats:
                parts.append(got["stats"])
        sums = torch.cat(parts, dim=1) if _stats else None                        # [nA, E, S, 6]
        staged = AsyncHost(sums) if (defer and _stats) else None

        def finish():
            r = {k: (v.cpu().numpy() if as_np else v) for k, v in res.items()}
            if not _stats:
                return r
            m = (staged.get() if staged is not None else sums.cpu()).numpy().astype(np.float64)       # ONE host read-back
            tot = np.zeros((nA, S, m.shape[-1]))
            for e in range(E):                                                    # environment order, whatever the chunks were
                tot += m[:, e]
            egos, pairs = tot[..., 0], tot[..., 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                r["stats"] = {"gate": np.where(pairs > 0, tot[..., 2] / pairs, np.nan),
                              "attention_per_ego": np.where(egos > 0, tot[..., 3] / egos, np.nan),
                              "present_mass": np.where(egos > 0, tot[..., 4] / egos, np.nan),
                              "entropy": np.where(egos > 0, tot[..., 5] / egos, np.nan),
                              "egos": egos, "pairs": pairs}
            return r
        return finish if defer else finish()

    # ---------------------------------------------------------------------------- attention saliency
    def _gat_saliency_chunk(self, who, N, through, max_workspace_mb):
        """rows (one scene per agent each) per chunk of a training-form GAT forward + ``ops.gat_saliency``, such that the record,
        the scratch and the noise the chunk holds while it is in flight stay under ``max_workspace_mb``"""
        nA, A = self.n_agents, self.args.attention_dim
        per_row = 4 * nA * (2 * ((N + 15) // 16) * (N - 1) * 2048 + N * (8 * A + 2 * (N - 1)) + 2 * N * (N - 1)
                            + (ops.gat_saliency_scratch_floats(1, 1, N) if through else 0))
        chunk = int(max_workspace_mb * (1 << 20)) // per_row
        if chunk < 1:
            raise ValueError(f"{who}: max_workspace_mb={max_workspace_mb} is too small for one row ({per_row / (1 << 20):.1f} MB)")
        return chunk

    def _gat_saliency_chunks(self, chunk, src0, lat, hid, noise, deterministic, tau, v, through, out, before=None, after=None):
        """``chunk`` rows [nA, b0:b1] at a time: the training form of the GAT forward on src0 / lat / hid with the chunk's noise (the
        record the backward reads), then ``ops.gat_saliency`` with the rows of ``v`` into the rows of the tensors in ``out`` (a dict
        by output name).  ``before(b0, b1, noise)`` runs ahead of the two launches (``v`` may be what it writes), ``after(b0, b1,
        record)`` behind them"""
        nA, B, N, _ = src0.shape
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            nz = self._noise(noise, deterministic, nA, b0, b1, (N, N - 1, 2))
            if before is not None:
                before(b0, b1, nz)
            _, saved = ops.gat_forward(self.gat_arena, src0[:, b0:b1], None if lat is None else lat[:, b0:b1], hid[:, b0:b1], nz, tau=tau,
                                       save=True)
            ops.gat_saliency(self.gat_arena, saved, v[:, b0:b1], gate_through=through, want=tuple(out),
                             out={k: t[:, b0:b1] for k, t in out.items()})
            if after is not None:
                after(b0, b1, saved)

    def attention_saliency(self, history, behavior_latent=None, hidden=None, target="self", noise=None, deterministic=True,
                           gate="through", tau=None, want=("pair",), max_workspace_mb=256):
        """How much do the inputs of entity j move the attention latent of ego i?  For every row (env, step, agent) of ``history``
        [E,S,nA,N,d] (with ``behavior_latent`` [E,S,nA,N,Z]; needed with ``GAT_use_behavior``, ignored without) and every ego i:
            y_i = <v_i, latent_i>,  latent = GAT([history || behavior_latent], hidden),  G[i, j, c] = d y_i / d obs[j, c]
        for every entity j, the ego included, and every column c of [hist || beh].  ``hidden`` [E,S,nA,N,A] is the state each row
        starts from (None: zeros; for a recorded batch ``attention_latent[:, :-1]`` with ``attention_trace``'s alignment); it is
        held constant, so the rows are independent and nothing is differentiated through time.
        ``target``: "self" -> v_i = latent_i (the gradient of 1/2 |latent_i|^2); an int -> the one-hot of that unit; a tensor
        [E,S,nA,N,A] -> used as given (e.g. the ``att`` columns of ``DcntrlMAC.saliency``'s ``actor_input_grad``).
        ``deterministic=True`` uses no gumbel noise and draws nothing (the gate is sigmoid((l1 - l0) / tau)); otherwise ``noise``
        [nA,E,S,N,N-1,2] is used, or drawn from torch's generator.  ``gate``: "through" = the exact derivative, 1/tau included;
        "held" = the gate is a constant (only the soft attention, the values and the output cell are differentiated).  ``tau``:
        None = the policy's own 0.01.
        Returns a dict; the pair tensors are indexed [ego i, entity j], n_src = 2 with ``GAT_use_behavior`` else 1:
          ``pair_gl1``, ``pair_gxi`` [E,S,nA,N,N,n_src]  sum_c |G[i,j,c]| and sum_c G[i,j,c] obs[j,c] per source ("pair" in ``want``)
          ``grad`` [E,S,nA,N,N,d+Z]                      all of G ("grad" in ``want``)
          ``input_grad`` [E,S,nA,N,d+Z]                  sum_i G[i,j,:] -- continues the policy's saliency to the GAT's inputs
          ``hidden_grad`` [E,S,nA,N,A]                   d y_i / d hidden_i
          ``latent``, ``target_vector`` [E,S,nA,N,A]     the forward result (the rollout's bits) and the v used
          ``active_h``, ``active_v`` [E,S,nA,N,32] bool  the ReLU branches of ``encoding`` and ``v`` the backward used
        The rows go through the training-form GAT forward and ``iplan_gat_saliency`` in chunks whose record and scratch stay
        under ``max_workspace_mb`` (the pair-GRU record alone is 3.5 MB per scene at 55 entities); a row's bits do not depend
        on the chunking.  numpy in -> numpy out, device tensors in -> device tensors out.  Parameters, gradients, optimiser
        state and (with ``deterministic=True``) torch's generator are not touched."""
        as_np = isinstance(history, np.ndarray)
        dev = self.device
        hist = _as_dev(history, dev)
        if hist.dim() != 5:
            raise ValueError(f"attention_saliency: history must be [E,S,nA,N,d], got {tuple(hist.shape)}")
        E, S, nA, N, d = hist.shape
        A = self.args.attention_dim
        if nA != self.n_agents or d != self.obs_shape or not 2 <= N <= ops.L.GAT_MAX_ENTITIES:
            raise ValueError(f"attention_saliency: history {tuple(hist.shape)} does not fit n_agents={self.n_agents}, obs width {self.obs_shape}, "
                             f"2 <= N <= {ops.L.GAT_MAX_ENTITIES}")
        if gate not in ("through", "held"):
            raise ValueError(f"attention_saliency: gate={gate!r} is neither 'through' nor 'held'")
        want = tuple(want)
        if any(k not in ("pair", "grad") for k in want):
            raise ValueError(f"attention_saliency: want={want} -- known: 'pair', 'grad'")
        if deterministic and noise is not None:
            raise ValueError("attention_saliency: noise was given together with deterministic=True")
        tau = 0.01 if tau is None else float(tau)
        if not tau > 0:
            raise ValueError(f"attention_saliency: tau={tau} must be positive")
        B = E * S
        Z = self.args.latent_dim if self.args.GAT_use_behavior else 0
        lat = self._beh_latent("attention_saliency", behavior_latent, (E, S, nA, N, Z))
        if lat is not None:
            lat = lat.permute(2, 0, 1, 3, 4).reshape(nA, B, N, Z).contiguous()
        D = d + Z
        n_src = 2 if Z else 1
        src0 = hist.permute(2, 0, 1, 3, 4).reshape(nA, B, N, d).contiguous()          # rows (agent, env * S + step): data movement only
        if hidden is None:
            hid = torch.zeros(nA, B, N, A, dtype=torch.float32, device=dev)
        else:
            hid = _as_dev(hidden, dev)
            if hid.shape != (E, S, nA, N, A):
                raise ValueError(f"attention_saliency: hidden {tuple(hid.shape)} != {(E, S, nA, N, A)}")
            hid = hid.permute(2, 0, 1, 3, 4).reshape(nA, B, N, A).contiguous()
        if noise is not None:
            noise = _as_dev(noise, dev)
            if noise.shape != (nA, E, S, N, N - 1, 2):
                raise ValueError(f"attention_saliency: noise {tuple(noise.shape)} != {(nA, E, S, N, N - 1, 2)}")
            noise = noise.reshape(nA, B, N, N - 1, 2)
        vt = None
        if isinstance(target, str):
            if target != "self":
                raise ValueError(f"attention_saliency: target={target!r} -- 'self', a unit index or a tensor [E,S,nA,N,A]")
        elif isinstance(target, (int, np.integer)) and not isinstance(target, bool):
            if not 0 <= int(target) < A:
                raise ValueError(f"attention_saliency: target unit {target} outside [0, {A})")
            vt = torch.zeros(nA, B, N, A, dtype=torch.float32, device=dev)
            vt[..., int(target)] = 1.0
        elif isinstance(target, (np.ndarray, torch.Tensor)):
            vt = _as_dev(target, dev)
            if vt.shape != (E, S, nA, N, A):
                raise ValueError(f"attention_saliency: target {tuple(vt.shape)} != {(E, S, nA, N, A)}")
            vt = vt.permute(2, 0, 1, 3, 4).reshape(nA, B, N, A).contiguous()
        else:
            raise ValueError(f"attention_saliency: target={target!r} -- 'self', a unit index or a tensor [E,S,nA,N,A]")
        through = gate == "through"
        chunk = self._gat_saliency_chunk("attention_saliency", N, through, max_workspace_mb)
        f32 = dict(dtype=torch.float32, device=dev)
        res = {"input_grad": torch.empty(nA, B, N, D, **f32), "hidden_grad": torch.empty(nA, B, N, A, **f32),
               "latent": torch.empty(nA, B, N, A, **f32)}
        if "pair" in want:
            res["pair_gl1"] = torch.empty(nA, B, N, N, n_src, **f32)
            res["pair_gxi"] = torch.empty(nA, B, N, N, n_src, **f32)
        if "grad" in want:
            res["grad"] = torch.empty(nA, B, N, N, D, **f32)
        res["target_vector"] = vt if vt is not None else res["latent"]
        act_h = torch.empty(nA, B, N, A, dtype=torch.bool, device=dev)
        act_v = torch.empty(nA, B, N, A, dtype=torch.bool, device=dev)

        def rollout_latent(b0, b1, nz):
            # the rollout's bits of the latent: the inference form of the forward (attention_map's launch)
            ops.gat_trace(self.gat_arena, src0[:, b0:b1].unsqueeze(2), None if lat is None else lat[:, b0:b1].unsqueeze(2), hid[:, b0:b1],
                          None if deterministic else nz.unsqueeze(2), tau=tau, want=("latent",), out={"latent": res["latent"][:, b0:b1].unsqueeze(2)})

        def active(b0, b1, saved):
            act_h[:, b0:b1] = saved["h_enc"].view(nA, b1 - b0, N, A) > 0
            act_v[:, b0:b1] = saved["qkv"].view(nA, b1 - b0, N, 3 * A)[..., 2 * A:] > 0
        self._gat_saliency_chunks(chunk, src0, lat, hid, noise, deterministic, tau, res["target_vector"], through,
                                  {k: res[k] for k in ops.GAT_SALIENCY_OUTPUTS if k in res}, before=rollout_latent, after=active)
        res["active_h"], res["active_v"] = act_h, act_v
        res = {k: v.unflatten(1, (E, S)).permute(1, 2, 0, *range(3, v.dim() + 1)) for k, v in res.items()}
        return {k: v.cpu().numpy() for k, v in res.items()} if as_np else res

    # ---------------------------------------------------------------------------- attention saliency through time
    def _gat_saliency_trace_plan(self, who, N, S, targets, K, through, deterministic, max_workspace_mb):
        """How ``attention_saliency_trace`` splits its work -> (environments per chunk, [(first, last + 1) target positions of each
        run]).  A chunk holds, per environment and agent, the training-form record and the noise of the steps its run of targets
        reaches, one scratch scene per target and (when the noise is sampled) the walk's noise over all S steps; that stays under
        ``max_workspace_mb``.  All targets in one run if at least one environment fits that way (then as many environments as
        fit); otherwise one environment per chunk and the targets in greedy runs."""
        nA, A = self.n_agents, self.args.attention_dim
        row = 2 * ((N + 15) // 16) * (N - 1) * 2048 + N * (8 * A + 2 * (N - 1)) + 2 * N * (N - 1)      # record + noise of one step
        scene = ops.gat_saliency_trace_scratch_floats(1, 1, 1, N) if through else 0
        walk = 0 if deterministic else S * 2 * N * (N - 1)

        def per_env(t0, t1):
            return 4 * nA * ((targets[t1 - 1] - max(0, targets[t0] - K) + 1) * row + (t1 - t0) * scene + walk)
        budget = int(max_workspace_mb * (1 << 20))
        T = len(targets)
        worst = max(per_env(t, t + 1) for t in range(T))
        if worst > budget:
            raise ValueError(f"{who}: max_workspace_mb={max_workspace_mb} is too small for one environment and one target with its "
                             f"{min(K, max(targets)) + 1}-step record ({worst / (1 << 20):.1f} MB)")
        if per_env(0, T) <= budget:
            return budget // per_env(0, T), [(0, T)]
        runs, t0 = [], 0
        while t0 < T:
            t1 = t0 + 1
            while t1 < T and per_env(t0, t1 + 1) <= budget:
                t1 += 1
            runs.append((t0, t1))
            t0 = t1
        return 1, runs

    def attention_saliency_trace(self, history, behavior_latent=None, hidden0=None, lags=0, targets=None, target="self", noise=None,
                                 deterministic=True, gate="through", tau=None, want=("pair",), presence_col=0, max_workspace_mb=256):
        """Ego i's social context at step s -- how much of it is owed to what vehicle j did k steps ago?  ``attention_saliency``
        through time.  The chain is ``attention_trace``'s: latent_s = GAT([history_s || behavior_latent_s], latent_{s-1}),
        latent_{-1} = ``hidden0`` [E,nA,N,A] (None: zeros), over ``history`` [E,S,nA,N,d] (with ``behavior_latent`` [E,S,nA,N,Z];
        needed with ``GAT_use_behavior``, ignored without).  For every target step s of ``targets`` (None: every step; else an
        ascending list of distinct steps -- the output axis T), ego i and lag k = 0 .. ``lags`` (an int in [0, S-1]):
            y_{s,i} = <v_{s,i}, latent_{s,i}>,   G^(k)[i, j, c] = d y_{s,i} / d obs_{s-k}[j, c],   c^(k)[i] = d y_{s,i} / d latent_{s-k-1,i}
        -- total derivatives through the ego's own latent chain (the output cell reads no other entity's latent, so there is no
        other path through time); for k = s the carry c^(k) is d y / d hidden0.  Lags with s - k < 0 do not exist: their slots
        are +0.0 and ``lag_valid`` is False.
        ``target``: "self" -> v = latent_s; an int -> the one-hot of that unit; a tensor [E,T,nA,N,A] -> used as given (e.g. the
        ``att`` columns of ``DcntrlMAC.saliency``'s ``actor_input_grad`` at the target steps).  ``deterministic``, ``noise``
        [nA,E,S,N,N-1,2], ``gate`` and ``tau`` as in ``attention_saliency``.
        Returns a dict, pair tensors indexed [ego i, entity j], n_src = 2 with ``GAT_use_behavior`` else 1:
          ``pair_gl1``, ``pair_gxi`` [E,T,K+1,nA,N,N,n_src]   per lag, as ``attention_saliency`` defines them ("pair" in ``want``)
          ``grad`` [E,T,K+1,nA,N,N,d+Z]                       all of G^(k) ("grad" in ``want``)
          ``input_grad`` [E,T,K+1,nA,N,d+Z]                   sum_i G^(k)[i,j,:]
          ``carry_l2`` [E,T,K+1,nA,N]                         |c^(k)[i]|;  ``carry`` [E,T,K+1,nA,N,A] with "carry" in ``want``
          ``lag_valid`` [T,K+1] bool, ``targets`` [T], ``target_vector`` [E,T,nA,N,A], ``latent`` [E,S,nA,N,A] (``attention_trace``'s bits)
          ``active_h``, ``active_v`` [E,S,nA,N,32] bool       the ReLU branches the backward used (False at steps no target reaches)
          ``lag_l1`` [nA,K+1,n_src,2] float64, ``lag_pairs`` [nA,K+1,2]  ("pair" in ``want``) per lag the mean of ``pair_gl1`` over the
                                                              counting pairs and their number, split into (i != j, i == j): "how far
                                                              back does the social context look".  A pair counts when the lag exists,
                                                              ego i is present at step s and entity j at step s - k (column
                                                              ``presence_col`` of its history row non-zero; < 0: everything counts);
                                                              nothing counting gives NaN.  Summed in float64 per environment from the
                                                              outputs in a stated order (entities, then egos, then targets, each axis
                                                              by pairwise halving), ONE read-back, environments added in order: a host
                                                              restatement of that order gives the same bits.
        Per chunk (a group of environments times a run of targets, see ``max_workspace_mb``): one ``iplan_gat_trace`` walk per
        group of environments, one training-form forward over the steps the run reaches with the walk's cat(hidden0, latent[:-1])
        as its previous state -- formed once, read by every target and lag -- and one ``iplan_gat_saliency_trace`` launch.  A
        slot's bits do not depend on the chunking, the other targets, ``lags`` or ``want``.  ``max_workspace_mb``: the default is small for
        many entities -- near N = 55 one environment's record of lags + 1 steps nearly fills it, a chunk is then one environment and a
        target or two, its few workgroups walk their lags in series, and the call is slower than lags + 1 ``attention_saliency`` calls
        (profiles/r30_attention_saliency_trace_notes.md); raise it (e.g. 8192) where the memory is there.  numpy in -> numpy out.  Parameters,
        gradients, optimiser state and (with ``deterministic=True``) torch's generator are not touched."""
        who = "attention_saliency_trace"
        as_np = isinstance(history, np.ndarray)
        dev = self.device
        hist = _as_dev(history, dev)
        if hist.dim() != 5:
            raise ValueError(f"{who}: history must be [E,S,nA,N,d], got {tuple(hist.shape)}")
        E, S, nA, N, d = hist.shape
        A = self.args.attention_dim
        if nA != self.n_agents or d != self.obs_shape or not 2 <= N <= ops.L.GAT_MAX_ENTITIES or E < 1 or S < 1:
            raise ValueError(f"{who}: history {tuple(hist.shape)} does not fit n_agents={self.n_agents}, obs width {self.obs_shape}, "
                             f"2 <= N <= {ops.L.GAT_MAX_ENTITIES}")
        if gate not in ("through", "held"):
            raise ValueError(f"{who}: gate={gate!r} is neither 'through' nor 'held'")
        want = tuple(want)
        if any(k not in ("pair", "grad", "carry") for k in want):
            raise ValueError(f"{who}: want={want} -- known: 'pair', 'grad', 'carry'")
        if deterministic and noise is not None:
            raise ValueError(f"{who}: noise was given together with deterministic=True")
        tau = 0.01 if tau is None else float(tau)
        if not tau > 0:
            raise ValueError(f"{who}: tau={tau} must be positive")
        if isinstance(lags, bool) or not isinstance(lags, (int, np.integer)) or not 0 <= int(lags) <= S - 1:
            raise ValueError(f"{who}: lags={lags!r} must be an int in [0, S-1={S - 1}]")
        K = int(lags)
        if targets is None:
            tg = list(range(S))
        else:
            given = list(targets)                                                 # (read once: a generator would be spent after it)
            ok = bool(given) and all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) and 0 <= t < S for t in given)
            if not ok or any(b <= a for a, b in zip(given, given[1:])):
                raise ValueError(f"{who}: targets={given} must be an ascending list of distinct steps in [0, {S})")
            tg = [int(t) for t in given]
        T = len(tg)
        if isinstance(presence_col, bool) or not isinstance(presence_col, (int, np.integer)) or presence_col >= d:
            raise ValueError(f"{who}: presence_col={presence_col!r} must be an int below the history's {d} columns (< 0: everything counts)")
        Z = self.args.latent_dim if self.args.GAT_use_behavior else 0
        lat = self._beh_latent(who, behavior_latent, (E, S, nA, N, Z))
        if lat is not None:
            lat = lat.permute(2, 0, 1, 3, 4)
        D, n_src = d + Z, 2 if Z else 1
        if hist.stride(4) != 1 or hist.stride(3) != d:
            hist = hist.contiguous()
        src0 = hist.permute(2, 0, 1, 3, 4)                                        # [nA, E, S, N, d] view
        f32 = dict(dtype=torch.float32, device=dev)
        if hidden0 is None:
            h0 = torch.zeros(nA, E, N, A, **f32)
        else:
            h0 = _as_dev(hidden0, dev)
            if h0.shape != (E, nA, N, A):
                raise ValueError(f"{who}: hidden0 {tuple(h0.shape)} != {(E, nA, N, A)}")
            h0 = h0.permute(1, 0, 2, 3).contiguous()
        if noise is not None:
            noise = _as_dev(noise, dev)
            if noise.shape != (nA, E, S, N, N - 1, 2):
                raise ValueError(f"{who}: noise {tuple(noise.shape)} != {(nA, E, S, N, N - 1, 2)}")
        vt = None
        if isinstance(target, str):
            if target != "self":
                raise ValueError(f"{who}: target={target!r} -- 'self', a unit index or a tensor [E,T,nA,N,A]")
        elif isinstance(target, (int, np.integer)) and not isinstance(target, bool):
            if not 0 <= int(target) < A:
                raise ValueError(f"{who}: target unit {target} outside [0, {A})")
            vt = torch.zeros(nA, E, T, N, A, **f32)
            vt[..., int(target)] = 1.0
        elif isinstance(target, (np.ndarray, torch.Tensor)):
            vt = _as_dev(target, dev)
            if vt.shape != (E, T, nA, N, A):
                raise ValueError(f"{who}: target {tuple(vt.shape)} != {(E, T, nA, N, A)}")
            vt = vt.permute(2, 0, 1, 3, 4).contiguous()
        else:
            raise ValueError(f"{who}: target={target!r} -- 'self', a unit index or a tensor [E,T,nA,N,A]")
        through = gate == "through"
        e_chunk, runs = self._gat_saliency_trace_plan(who, N, S, tg, K, through, deterministic, max_workspace_mb)

        latent = torch.empty(E, S, nA, N, A, **f32)
        lat_w = latent.permute(2, 0, 1, 3, 4)                                     # [nA, E, S, N, A] view the walk writes
        outs = {"input_grad": torch.empty(nA, E, T, K + 1, N, D, **f32), "carry_sq": torch.empty(nA, E, T, K + 1, N, **f32)}
        if "pair" in want:
            outs["pair_gl1"] = torch.empty(nA, E, T, K + 1, N, N, n_src, **f32)
            outs["pair_gxi"] = torch.empty(nA, E, T, K + 1, N, N, n_src, **f32)
        if "grad" in want:
            outs["grad"] = torch.empty(nA, E, T, K + 1, N, N, D, **f32)
        if "carry" in want:
            outs["carry"] = torch.empty(nA, E, T, K + 1, N, A, **f32)
        if vt is None:
            vt = torch.empty(nA, E, T, N, A, **f32)
            self_target = True
        else:
            self_target = False
        act_h = torch.zeros(nA, E, S, N, A, dtype=torch.bool, device=dev)
        act_v = torch.zeros(nA, E, S, N, A, dtype=torch.bool, device=dev)
        # a run's targets as record steps, on the device: the same for every group of environments, uploaded once
        run_tg = [[s - max(0, tg[t0] - K) for s in tg[t0:t1]] for t0, t1 in runs]
        run_dev = [torch.tensor(r, dtype=torch.int32, device=dev) for r in run_tg]
        for e0 in range(0, E, e_chunk):
            e1 = min(E, e0 + e_chunk)
            Ee = e1 - e0
            nz = self._noise(noise, deterministic, nA, e0, e1, (S, N, N - 1, 2), zeros=False)
            ops.gat_trace(self.gat_arena, src0[:, e0:e1], None if lat is None else lat[:, e0:e1], h0[:, e0:e1], nz, tau=tau,
                          want=("latent",), out={"latent": lat_w[:, e0:e1]})
            if self_target:
                vt[:, e0:e1] = lat_w[:, e0:e1, tg]
            for run, (t0, t1) in enumerate(runs):
                r0, r1 = max(0, tg[t0] - K), tg[t1 - 1] + 1                       # the record's steps r0 .. r1 - 1
                R = r1 - r0
                rows = lambda x: x[:, e0:e1, r0:r1].reshape(nA, Ee * R, *x.shape[3:])     # noqa: E731  (env, step) rows: data movement only
                if r0 == 0:
                    hprev = torch.cat([h0[:, e0:e1].unsqueeze(2), lat_w[:, e0:e1, :r1 - 1]], dim=2).reshape(nA, Ee * R, N, A)
                else:
                    hprev = lat_w[:, e0:e1, r0 - 1:r1 - 1].reshape(nA, Ee * R, N, A)
                nzr = torch.zeros(nA, Ee * R, N, N - 1, 2, **f32) if deterministic else nz[:, :, r0:r1].reshape(nA, Ee * R, N, N - 1, 2).contiguous()
                _, saved = ops.gat_forward(self.gat_arena, rows(src0).contiguous(), None if lat is None else rows(lat).contiguous(),
                                           hprev.contiguous(), nzr, tau=tau, save=True)
                ops.gat_saliency_trace(self.gat_arena, saved, R, vt[:, e0:e1, t0:t1], run_tg[run], K, gate_through=through, want=tuple(outs),
                                       out={k: t[:, e0:e1, t0:t1] for k, t in outs.items()}, targets_dev=run_dev[run])
                act_h[:, e0:e1, r0:r1] = saved["h_enc"].view(nA, Ee, R, N, A) > 0
                act_v[:, e0:e1, r0:r1] = saved["qkv"].view(nA, Ee, R, N, 3 * A)[..., 2 * A:] > 0
                del saved                                                         # (not held while the next chunk's record is formed)
        tgt = torch.tensor(tg, dtype=torch.int64)
        lag_valid = torch.arange(K + 1)[None, :] <= tgt[:, None]                   # [T, K+1]
        sums = None
        if "pair" in want:
            # per environment, in float64 where the outputs lie: the sums of pair_gl1 and the counts over the counting pairs
            step_j = (tgt[:, None] - torch.arange(K + 1)[None, :]).clamp(min=0).to(dev)
            tgt_d, valid_d = tgt.to(dev), lag_valid.to(dev)
            eye = torch.eye(N, dtype=torch.bool, device=dev)
            parts = []
            for e in range(E):
                if presence_col >= 0:
                    pres = src0[:, e, :, :, presence_col] != 0                    # [nA, S, N]
                    m = pres[:, tgt_d][:, :, None, :, None] & pres[:, step_j][:, :, :, None, :]
                else:
                    m = torch.ones(nA, T, K + 1, N, N, dtype=torch.bool, device=dev)
                m = m & valid_d[None, :, :, None, None]
                g = outs["pair_gl1"][:, e].to(torch.float64)                      # [nA, T, K+1, N, N, n_src]
                split = [m & ~eye, m & eye]
                # in a stated order -- entities, then egos, then targets, each by pairwise halving -- so that a host restatement
                # of the same order gives the same bits (counts are integers: any order)
                tot = torch.stack([_halving_sum(_halving_sum(_halving_sum(g * s[..., None], 4), 3), 1) for s in split], dim=-1)   # [nA, K+1, n_src, 2]
                cnt = torch.stack([s.sum(dim=(1, 3, 4)).to(torch.float64) for s in split], dim=-1)                # [nA, K+1, 2]
                parts.append(torch.cat([tot, cnt[:, :, None, :]], dim=2))         # [nA, K+1, n_src + 1, 2]
            sums = torch.stack(parts)
        res = {k: v.permute(1, 2, 3, 0, *range(4, v.dim())) for k, v in outs.items()}
        res["carry_l2"] = torch.sqrt(res.pop("carry_sq"))
        res["latent"] = latent
        res["target_vector"] = vt.permute(1, 2, 0, 3, 4)
        res["active_h"], res["active_v"] = act_h.permute(1, 2, 0, 3, 4), act_v.permute(1, 2, 0, 3, 4)
        res["lag_valid"], res["targets"] = lag_valid, tgt
        if as_np:
            res = {k: v.cpu().numpy() for k, v in res.items()}
        if sums is not None:
            m = sums.cpu().numpy()                                                # ONE host read-back
            tot = np.zeros(m.shape[1:])
            for e in range(E):                                                    # environment order, whatever the chunks were
                tot += m[e]
            cnt = tot[:, :, n_src, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                res["lag_l1"] = np.where(cnt[:, :, None, :] > 0, tot[:, :, :n_src, :] / cnt[:, :, None, :], np.nan)
            res["lag_pairs"] = cnt
        return res

    # ---------------------------------------------------------------------------- neighbour knock-out
    def _knock_spec(self, who, N, d, sources, want, noise, deterministic, tau, presence_col, entities, baseline):
        """the arguments ``attention_knockout`` and ``attention_knockout_trace`` share, checked (ValueError) and normalised ->
        (sources, knock flags per source, want, tau, the job list, the baseline rows [history, behaviour] on the device or None)"""
        sources = (sources,) if isinstance(sources, str) else tuple(sources)
        if not sources or any(s not in ("history", "behavior") for s in sources):
            raise ValueError(f"{who}: sources={sources} -- 'history', 'behavior' or both")
        if "behavior" in sources and not self.args.GAT_use_behavior:
            raise ValueError(f"{who}: sources={sources}, but this policy's GAT reads no behaviour latent (GAT_use_behavior is off)")
        knock = ("history" in sources, "behavior" in sources)
        want = tuple(want)
        if any(k not in ("shift", "latent_ko", "attention_ko") for k in want):
            raise ValueError(f"{who}: want={want} -- known: 'shift', 'latent_ko', 'attention_ko'")
        if deterministic and noise is not None:
            raise ValueError(f"{who}: noise was given together with deterministic=True")
        tau = 0.01 if tau is None else float(tau)
        if not tau > 0:
            raise ValueError(f"{who}: tau={tau} must be positive")
        if not isinstance(presence_col, (int, np.integer)) or presence_col >= d:
            raise ValueError(f"{who}: presence_col={presence_col!r} outside the {d} columns")
        if entities is None:
            entities = range(N)
        try:
            jobs = list(entities)
        except TypeError:
            raise ValueError(f"{who}: entities={entities!r} -- None or a list of entity indices") from None
        if not jobs or any(isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= j < N for j in jobs):
            raise ValueError(f"{who}: entities={jobs} -- ints in [0, {N}), at least one")
        jobs = [int(j) for j in jobs]
        Z = self.args.latent_dim if self.args.GAT_use_behavior else 0
        rows = [None, None]
        if baseline is not None:
            if not isinstance(baseline, (tuple, list)) or len(baseline) != 2:
                raise ValueError(f"{who}: baseline -- None or a pair (row [{d}] or None, row [{Z}] or None)")
            for s, (row, width) in enumerate(zip(baseline, (d, Z))):
                if row is None:
                    continue
                row = _as_dev(torch.as_tensor(row), self.device).contiguous()
                if row.shape != (width,) or width == 0:
                    raise ValueError(f"{who}: baseline[{s}] {tuple(row.shape)} != {(width,)}")
                rows[s] = row
        return sources, knock, want, tau, jobs, rows

    def attention_knockout(self, history, behavior_latent=None, hidden=None, entities=None, sources=("history", "behavior"), baseline=None,
                           noise=None, deterministic=True, tau=None, want=("shift",), forecast=False, pos=(1, 2), presence_col=0,
                           max_workspace_mb=256):
        """What becomes of ego i's social context, and of its forecast, if vehicle j were not there?  Occlusion (leave-one-out)
        attribution of the GAT: for every row (env, step, agent) of ``history`` [E,S,nA,N,d] (with ``behavior_latent`` [E,S,nA,N,Z];
        needed with ``GAT_use_behavior``, ignored without) and every entity j of ``entities`` (default: all N; duplicates allowed), the
        GAT is run again with entity j's input row replaced (``iplan_gat_knockout``: one workgroup per row and j, inputs read in place).
        ``hidden`` [E,S,nA,N,A] is the state each row starts from (None: zeros; for a recorded batch ``attention_latent[:, :-1]``); it
        is held -- entity j's hidden row is not changed -- and nothing is carried through time, as in ``attention_saliency``.
        ``sources``: what "not there" means -- ("history", "behavior") = the vehicle is unseen, ("behavior",) = the ego does not know
        j's intent, ("history",) = only the observation row.  ``baseline``: None = zeros for both (for history the observation wrapper's
        encoding of an unseen vehicle), or a pair (row [d] or None, row [Z] or None).  ``deterministic=True`` uses no gumbel noise and
        draws nothing; otherwise ``noise`` [nA,E,S,N,N-1,2] (or a draw from torch's generator) is used for the base AND for every knocked
        run (common random numbers).  ``tau``: None = the policy's own 0.01.
        Returns a dict; pair tensors are indexed [ego i, knocked entity], J = len(entities):
          ``latent`` [E,S,nA,N,A]           nothing knocked: bit for bit ``GAT_latent_update``'s on the same noise
          ``latent_shift`` [E,S,nA,N,J]     with "shift" in ``want`` (the default): ||latent_ko[j][i] - latent[i]||_2, torch's sqrt of the
                                            kernel's sum of squares (columns ascending, every product and sum rounded on its own)
          ``knocked``                       the entity list (int64 numpy [J])
          ``latent_ko`` [E,S,nA,J,N,A], ``attention_ko`` [E,S,nA,J,N,N]   with "latent_ko" / "attention_ko" in ``want``: the knocked
                                            latents and entity-indexed soft * hard maps (``attention_map``'s ``attention`` on the modified copy)
          ``summary`` float64 numpy [nA,2]  with "shift": after ONE read-back (without "shift" nothing is read back): [:, 0] the mean of latent_shift over pairs i != j with both present, [:, 1]
                                            over i == j with i present (column ``presence_col`` of the history row non-zero; < 0: everything
                                            counts); NaN where nothing counts
        ``forecast=True`` sends the knocked latents through the decoder (``iplan_predict``; its start state is read in place and never
        knocked, so the result isolates the social path) and adds ``pred`` [E,S,nA,N,P,d], bit for bit ``predict``'s, and
        ``forecast_shift`` [E,S,nA,N,J,P]: the Euclidean distance over the ``pos`` columns between entity i's forecast with and without
        j, formed in torch -- the squared differences of the columns added in ``pos`` order, then sqrt.
        Rows and jobs are chunked so that what a chunk holds in flight stays under ``max_workspace_mb``; the bits do not depend on the
        chunking.  numpy in -> numpy out, device tensors in -> device tensors out.  Parameters, gradients, optimiser state, carried
        state and (with ``deterministic=True``) torch's generator are not touched.  Not covered: deleting an entity from the pair chain
        (the row is replaced, which is what the environment would have shown), knocking the hidden state, continuation into the
        actors and critics, aggregation across data-parallel ranks (effects carried through time: ``attention_knockout_trace``)."""
        who = "attention_knockout"
        as_np = isinstance(history, np.ndarray)
        dev = self.device
        hist = _as_dev(history, dev)
        if hist.dim() != 5:
            raise ValueError(f"{who}: history must be [E,S,nA,N,d], got {tuple(hist.shape)}")
        E, S, nA, N, d = hist.shape
        A, P = self.args.attention_dim, self.pred_length
        if nA != self.n_agents or d != self.obs_shape or not 2 <= N <= ops.L.GAT_MAX_ENTITIES:
            raise ValueError(f"{who}: history {tuple(hist.shape)} does not fit n_agents={self.n_agents}, obs width {self.obs_shape}, "
                             f"2 <= N <= {ops.L.GAT_MAX_ENTITIES}")
        sources, knock, want, tau, jobs, rows = self._knock_spec(who, N, d, sources, want, noise, deterministic, tau, presence_col, entities, baseline)
        J = len(jobs)
        pos = tuple(pos) if forecast else ()
        if forecast and (not pos or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < d for c in pos)):
            raise ValueError(f"{who}: pos={pos} -- columns in [0, {d}), at least one")
        B = E * S
        Z = self.args.latent_dim if self.args.GAT_use_behavior else 0
        if hist.stride(4) != 1 or hist.stride(3) != d:
            hist = hist.contiguous()
        src0 = hist.permute(2, 0, 1, 3, 4).reshape(nA, B, N, d)                   # rows (agent, env * S + step): a view where the layout allows
        lat = self._beh_latent(who, behavior_latent, (E, S, nA, N, Z))
        if lat is not None:
            if lat.stride(4) != 1 or lat.stride(3) != Z:
                lat = lat.contiguous()
            lat = lat.permute(2, 0, 1, 3, 4).reshape(nA, B, N, Z)
        if hidden is None:
            hid = torch.zeros(nA, B, N, A, dtype=torch.float32, device=dev)
        else:
            hid = _as_dev(hidden, dev)
            if hid.shape != (E, S, nA, N, A):
                raise ValueError(f"{who}: hidden {tuple(hid.shape)} != {(E, S, nA, N, A)}")
            hid = hid.permute(2, 0, 1, 3, 4).reshape(nA, B, N, A).contiguous()
        if noise is not None:
            noise = _as_dev(noise, dev)
            if noise.shape != (nA, E, S, N, N - 1, 2):
                raise ValueError(f"{who}: noise {tuple(noise.shape)} != {(nA, E, S, N, N - 1, 2)}")
            noise = noise.reshape(nA, B, N, N - 1, 2)
        keep_shift, keep_lat, keep_attn = "shift" in want, "latent_ko" in want, "attention_ko" in want
        if not (keep_shift or keep_lat or keep_attn or forecast):
            raise ValueError(f"{who}: want={want} without forecast=True asks for nothing")
        # what a chunk holds in flight, in bytes per row (all agents): the noise and the base latent (and forecast), and per (row, job)
        # the knocked outputs (and forecasts)
        per_row = 4 * nA * (2 * N * (N - 1) + N * A + (N * P * d if forecast else 0))
        per_job = 4 * nA * ((N if keep_shift else 0) + (N * A if keep_lat or forecast else 0) + (N * N if keep_attn else 0) + (N * P * (d + 1) if forecast else 0))
        budget = int(max_workspace_mb * (1 << 20))
        if budget < per_row + per_job:
            raise ValueError(f"{who}: max_workspace_mb={max_workspace_mb} is too small for one row and one job "
                             f"({(per_row + per_job) / (1 << 20):.2f} MB)")
        jc = min(J, (budget - per_row) // per_job)
        rc = min(B, budget // (per_row + jc * per_job))
        f32 = dict(dtype=torch.float32, device=dev)
        res = {"latent": torch.empty(nA, B, N, A, **f32)}
        if keep_shift:
            res["shift_sq"] = torch.empty(nA, B, J, N, **f32)
        if keep_lat:
            res["latent_ko"] = torch.empty(nA, B, J, N, A, **f32)
        if keep_attn:
            res["attention_ko"] = torch.empty(nA, B, J, N, N, **f32)
        if forecast:
            res["pred"] = torch.empty(nA, B, N, P, d, **f32)
            res["forecast_shift"] = torch.empty(nA, B, J, N, P, **f32)
            row_off = (torch.arange(nA)[:, None] * src0.stride(0) + torch.arange(B)[None, :] * src0.stride(1)).to(torch.int64)
            assert int(row_off.max()) + (N - 1) * src0.stride(2) + d <= ops._room(src0)
            row_off = row_off.to(dev)
        for b0 in range(0, B, rc):
            b1 = min(B, b0 + rc)
            nb = b1 - b0
            nz = self._noise(noise, deterministic, nA, b0, b1, (N, N - 1, 2))
            base = res["latent"][:, b0:b1]
            s1 = None if lat is None else lat[:, b0:b1]
            ops.gat_forward(self.gat_arena, src0[:, b0:b1], s1, hid[:, b0:b1], nz, tau=tau, out=base)      # the rollout's launch and bits
            if forecast:
                off_b = row_off[:, b0:b1].contiguous()
                pb = ops.predict(self.dec_arena, src0, off_b, src0.stride(2), 0, base.reshape(nA, nb * N, A).contiguous(), N, P, d,
                                 checked=True)["pred"]
                pb = pb.view(nA, nb, N, P, d)
                res["pred"][:, b0:b1] = pb
            for j0 in range(0, J, jc):
                j1 = min(J, j0 + jc)
                nj = j1 - j0
                out = {"shift_sq": res["shift_sq"][:, b0:b1, j0:j1]} if keep_shift else {}
                if forecast:
                    out["latent_ko"] = torch.empty(nA, nb, nj, N, A, **f32)     # contiguous: the decoder's h0
                elif keep_lat:
                    out["latent_ko"] = res["latent_ko"][:, b0:b1, j0:j1]
                if keep_attn:
                    out["attn_ko"] = res["attention_ko"][:, b0:b1, j0:j1]
                ops.gat_knockout(self.gat_arena, src0[:, b0:b1], s1, hid[:, b0:b1], jobs[j0:j1], base=base if keep_shift else None, noise=None if deterministic else nz,
                                 tau=tau, knock=knock, baseline=rows, want=tuple(out), out=out)
                if forecast:
                    if keep_lat:
                        res["latent_ko"][:, b0:b1, j0:j1] = out["latent_ko"]
                    off_j = off_b[:, :, None].expand(nA, nb, nj).reshape(nA, nb * nj).contiguous()
                    pk = ops.predict(self.dec_arena, src0, off_j, src0.stride(2), 0, out["latent_ko"].view(nA, nb * nj * N, A), N, P, d,
                                     checked=True)["pred"].view(nA, nb, nj, N, P, d)
                    # the squared differences of the position columns, added in `pos` order, then sqrt
                    acc = None
                    for c in pos:
                        diff = pk[..., c] - pb[:, :, None, :, :, c]
                        acc = diff * diff if acc is None else acc + diff * diff
                    res["forecast_shift"][:, b0:b1, j0:j1] = acc.sqrt()
        shift = res.pop("shift_sq").sqrt() if keep_shift else None                 # [nA, B, J, N]

        def rows_out(t, pair=False):                                               # [nA, B, ...] -> [E, S, nA, ...]; pair: [J, N, ..] -> [N, J, ..]
            t = t.unflatten(1, (E, S)).permute(1, 2, 0, *range(3, t.dim() + 1))
            return t.transpose(3, 4) if pair else t
        final = {"latent": rows_out(res["latent"])}
        if keep_shift:
            final["latent_shift"] = rows_out(shift, pair=True)
        if keep_lat:
            final["latent_ko"] = rows_out(res["latent_ko"])
        if keep_attn:
            final["attention_ko"] = rows_out(res["attention_ko"])
        if forecast:
            final["pred"] = rows_out(res["pred"])
            final["forecast_shift"] = rows_out(res["forecast_shift"], pair=True)
        jn = np.asarray(jobs, dtype=np.int64)
        if keep_shift:
            # the two means per agent: ONE host read-back of the shifts and the presence flags
            present = (src0[..., presence_col] != 0) if presence_col >= 0 else torch.ones(nA, B, N, dtype=torch.bool, device=dev)
            host = torch.cat([shift, present[:, :, None, :].to(torch.float32)], dim=2).cpu().numpy().astype(np.float64)      # [nA, B, J + 1, N]
            sh, pr = host[:, :, :J], host[:, :, J] != 0                                # [nA, B, J, N], [nA, B, N]
            own = jn[:, None] == np.arange(N)[None, :]                                 # [J, N]: slot j knocks ego i itself
            other = pr[:, :, None, :] & pr[:, :, jn][:, :, :, None] & ~own[None, None]
            self_ = pr[:, :, None, :] & own[None, None]
            summary = np.full((nA, 2), np.nan)
            for col, m in enumerate((other, self_)):
                cnt = m.sum(axis=(1, 2, 3)).astype(np.float64)
                tot = np.where(m, sh, 0.0).sum(axis=(1, 2, 3))
                summary[:, col] = np.where(cnt > 0, tot / np.maximum(cnt, 1.0), np.nan)
        final = {k: (v.cpu().numpy() if as_np else v) for k, v in final.items()}
        final["knocked"] = jn
        if keep_shift:
            final["summary"] = summary
        return final

    def attention_knockout_trace(self, history, behavior_latent=None, hidden0=None, entities=None, start=0, duration=1, horizon=None,
                                 sources=("history", "behavior"), baseline=None, noise=None, deterministic=True, tau=None, want=("shift",),
                                 presence_col=0, max_workspace_mb=256, forecast=False, pos=(1, 2)):
        """How long does the social context remember a vehicle?  Vehicle j is out of sight for ``duration`` = D steps from step
        ``start`` and visible again afterwards; the GAT walks steps start .. start + H - 1 (``horizon`` = H, None: up to the last step
        of ``history``; ``duration`` None: knocked throughout, D = H) once per entity j of ``entities`` (default: all N; duplicates
        allowed) and once with nothing knocked, every chain carrying its OWN latent: latent_s = GAT(history_s, behavior_latent_s,
        latent_{s-1}).  In the first D steps entity j's input row is replaced as ``attention_knockout`` replaces it; the later steps
        see the recorded rows, and only the chain's carried latent remembers the knock (the echo).  ``history`` [E,S,nA,N,d] and
        ``behavior_latent`` [E,S,nA,N,Z] (needed with ``GAT_use_behavior``, ignored without) are aligned as in ``attention_trace``
        and read in place; ``hidden0`` [E,nA,N,A] is the state step ``start`` starts from (None: zeros) -- for a replayed rollout with
        ``attention_trace``'s alignment (``history[:, 1:]``, ``behavior_latent[:, :-1]``) that is ``attention_latent[:, start]``.
        Entity j's hidden row is never overwritten.  ``sources``, ``baseline``, ``entities``, ``tau``, ``noise`` and ``deterministic``
        mean what they mean in ``attention_knockout``; ``noise`` is [nA,E,H,N,N-1,2], the window's samples, used for the base walk AND
        for every knocked chain (common random numbers).
        Per chunk of environments one ``iplan_gat_trace`` launch walks the window with nothing knocked, then ``iplan_gat_knockout_trace``
        (one workgroup per (agent, env, job) for the whole window) walks the jobs.  Returns a dict; pair tensors are indexed [ego i,
        knocked entity], J = len(entities):
          ``latent`` [E,H,nA,N,A]           nothing knocked: bit for bit ``attention_trace``'s on the window
          ``latent_shift`` [E,H,nA,N,J]     with "shift" in ``want`` (the default): ||latent_ko[j][i] - latent[i]||_2 per step, torch's sqrt
                                            of the kernel's sum of squares (columns ascending, every product and sum rounded on its own)
          ``knocked``, ``sources``, ``window``   the entity list (int64 numpy [J]), the sources, (start, D, H)
          ``latent_ko`` [E,H,nA,J,N,A], ``attention_ko`` [E,H,nA,J,N,N]   with "latent_ko" / "attention_ko" in ``want``: the knocked chains'
                                            latents and entity-indexed soft * hard maps (``attention_trace``'s on the modified copy)
          ``summary`` float64 numpy [nA,H,2]   with "shift", after ONE read-back: per step of the window the mean of latent_shift over
                                            pairs i != j ([..., 0]) and over i == j ([..., 1]).  A pair counts at step h when ego i is
                                            present at step start + h and entity j is present in at least one knocked step (column
                                            ``presence_col`` of the history row non-zero; < 0: everything counts); the environments are
                                            added in environment order; NaN where nothing counts
        ``forecast=True`` answers the occlusion question for the forecasts: how far do every ego's forecasts of the scene move while
        j is out of sight and afterwards, and how much worse do they get against what then happened?  Per chunk one ``iplan_predict``
        launch decodes the base walk's latents, and ``iplan_predict_knockout`` decodes every knocked chain's latent at every step of
        the window where the walk wrote it, reducing each forecast to P numbers per pair and step in the kernel; the decoder's start
        state, ``history[:, start + h]``, is read in place and never knocked (``attention_knockout``'s rule: the result isolates the
        social path), the targets are ``history[:, start + h + 1 + p]``.  ``want`` may then be empty of the names above and accepts
        "forecast_error" and "pred_ko" (ValueError without ``forecast=True``).  ``pos``: the columns of the distance, distinct, added
        in the order given.  It adds, P = ``pred_length``:
          ``pred`` [E,H,nA,N,P,d]           nothing knocked: bit for bit ``ops.predict`` on the window's ``latent``
          ``forecast_shift`` [E,H,nA,N,J,P] the Euclidean distance over the ``pos`` columns between entity i's forecast with and without
                                            j: torch's sqrt of the kernel's sum of squares (every difference, product and sum rounded
                                            on its own; at H = D = 1 bit for bit ``attention_knockout(forecast=True)``'s)
          ``forecast_summary`` float64 numpy [nA,H,P,2]   the mean of forecast_shift over pairs i != j and over i == j under ``summary``'s
                                            counting rule, from float64 sums formed on the device per (agent, env, step, p) and added
                                            over the environments on the host in environment order; NaN where nothing counts.
                                            All summaries of a call share ONE read-back
          with "forecast_error": ``forecast_error`` [E,H,nA,N,P] and ``forecast_error_ko`` [E,H,nA,N,J,P], the same distance between the
                                            forecast (base, knocked) and the recorded future, +0.0 where the target step is not
                                            recorded; ``forecast_valid`` bool numpy [H,P]: the target step start + h + 1 + p exists;
                                            ``forecast_error_summary`` float64 numpy [nA,H,P,2]: the mean base error and the mean knocked
                                            error over the pairs i != j that count, whose target exists and whose entity i is present
                                            in the target row
          with "pred_ko": ``pred_ko`` [E,H,nA,J,N,P,d]   the knocked chains' forecasts
        With ``forecast=False`` nothing changes: the same launches, bits and keys.
        Environments and jobs are chunked so that what a chunk holds in flight stays under ``max_workspace_mb``; the bits do not depend
        on the chunking.  numpy in -> numpy out, device tensors in -> device tensors out.  Parameters, gradients, optimiser state,
        carried state and (with ``deterministic=True``) torch's generator are not touched.  Not covered: knocking the hidden state
        or the decoder's start state, a chain into ``evaluate``'s sampling, horizon subsets, aggregation across data-parallel ranks.
        ``latent_ko`` over steps continues into the policy as ``DcntrlMAC.knockout_trace``'s per-job override; its ``social=`` does
        both halves in one call."""
        who = "attention_knockout_trace"
        as_np = isinstance(history, np.ndarray)
        dev = self.device
        hist = _as_dev(history, dev)
        if hist.dim() != 5:
            raise ValueError(f"{who}: history must be [E,S,nA,N,d], got {tuple(hist.shape)}")
        E, S, nA, N, d = hist.shape
        A, P = self.args.attention_dim, self.pred_length
        if nA != self.n_agents or d != self.obs_shape or not 2 <= N <= ops.L.GAT_MAX_ENTITIES:
            raise ValueError(f"{who}: history {tuple(hist.shape)} does not fit n_agents={self.n_agents}, obs width {self.obs_shape}, "
                             f"2 <= N <= {ops.L.GAT_MAX_ENTITIES}")
        want = tuple(want)
        keep_err, keep_pk = "forecast_error" in want, "pred_ko" in want
        if (keep_err or keep_pk) and not forecast:
            raise ValueError(f"{who}: want={want} -- 'forecast_error' and 'pred_ko' need forecast=True")
        want = tuple(k for k in want if k not in ("forecast_error", "pred_ko"))
        sources, knock, want, tau, jobs, rows = self._knock_spec(who, N, d, sources, want, noise, deterministic, tau, presence_col, entities, baseline)
        J = len(jobs)
        ints = (int, np.integer)
        pos = tuple(pos) if forecast else ()
        if forecast and (not pos or any(isinstance(c, bool) or not isinstance(c, ints) or not 0 <= c < d for c in pos) or len(set(pos)) != len(pos)):
            raise ValueError(f"{who}: pos={pos} -- distinct columns in [0, {d}), at least one")
        if not isinstance(start, ints) or not 0 <= start < S:
            raise ValueError(f"{who}: start={start!r} outside [0, {S})")
        start = int(start)
        H = S - start if horizon is None else horizon
        if not isinstance(H, ints) or not 1 <= H or start + H > S:
            raise ValueError(f"{who}: horizon={horizon!r} must satisfy 1 <= horizon and start + horizon <= {S}")
        H = int(H)
        D = H if duration is None else duration
        if not isinstance(D, ints) or not 1 <= D <= H:
            raise ValueError(f"{who}: duration={duration!r} outside [1, horizon={H}]")
        D = int(D)
        keep_shift, keep_lat, keep_attn = "shift" in want, "latent_ko" in want, "attention_ko" in want
        if not (keep_shift or keep_lat or keep_attn or forecast):
            raise ValueError(f"{who}: want={want} asks for nothing")
        Z = self.args.latent_dim if self.args.GAT_use_behavior else 0
        if hist.stride(4) != 1 or hist.stride(3) != d:
            hist = hist.contiguous()
        src0 = hist.permute(2, 0, 1, 3, 4)                                        # [nA, E, S, N, d] view, read in place
        lat = self._beh_latent(who, behavior_latent, (E, S, nA, N, Z))
        if lat is not None:
            if lat.stride(4) != 1 or lat.stride(3) != Z:
                lat = lat.contiguous()
            lat = lat.permute(2, 0, 1, 3, 4)
        h0 = None
        if hidden0 is not None:
            h0 = _as_dev(hidden0, dev)
            if h0.shape != (E, nA, N, A):
                raise ValueError(f"{who}: hidden0 {tuple(h0.shape)} != {(E, nA, N, A)}")
            if h0.stride(3) != 1 or h0.stride(2) != A or h0.data_ptr() % 16 or h0.stride(0) % 4 or h0.stride(1) % 4:
                h0 = h0.contiguous()
            h0 = h0.permute(1, 0, 2, 3)
        if noise is not None:
            noise = _as_dev(noise, dev)
            if noise.shape != (nA, E, H, N, N - 1, 2):
                raise ValueError(f"{who}: noise {tuple(noise.shape)} != {(nA, E, H, N, N - 1, 2)}")
        # what a chunk holds in flight, in bytes per environment (all agents, the window): the noise and the base walk's latents, and
        # per (environment, job) the knocked chain's outputs
        per_env = 4 * nA * H * (2 * N * (N - 1) + N * A)
        per_job = 4 * nA * H * ((N if keep_shift else 0) + (N * A if keep_lat else 0) + (N * N if keep_attn else 0))
        if forecast:
            # the base forecasts (and errors) per environment; per (environment, job) the chain's latents -- a workspace unless they
            # are a result -- and P floats per pair and step per output, P d with the forecasts themselves
            per_env += 4 * nA * H * N * P * (d + (1 if keep_err else 0))
            per_job += 4 * nA * H * ((0 if keep_lat else N * A) + N * P * (2 if keep_err else 1) + (N * P * d if keep_pk else 0))
        budget = int(max_workspace_mb * (1 << 20))
        if budget < per_env + per_job:
            raise ValueError(f"{who}: max_workspace_mb={max_workspace_mb} is too small for one environment and one job "
                             f"({(per_env + per_job) / (1 << 20):.2f} MB)")
        jc = min(J, (budget - per_env) // per_job)
        ec = min(E, budget // (per_env + jc * per_job))
        f32 = dict(dtype=torch.float32, device=dev)
        res = {"latent": torch.empty(nA, E, H, N, A, **f32)}
        if keep_shift:
            res["shift_sq"] = torch.empty(nA, E, J, H, N, **f32)
        if keep_lat:
            res["latent_ko"] = torch.empty(nA, E, J, H, N, A, **f32)
        if keep_attn:
            res["attention_ko"] = torch.empty(nA, E, J, H, N, N, **f32)
        if forecast:
            res["pred"] = torch.empty(nA, E, H, N, P, d, **f32)
            res["fshift_sq"] = torch.empty(nA, E, J, H, N, P, **f32)
            if keep_err:
                res["ferr_base_sq"] = torch.empty(nA, E, 1, H, N, P, **f32)
                res["ferr_sq"] = torch.empty(nA, E, J, H, N, P, **f32)
            if keep_pk:
                res["pred_ko"] = torch.empty(nA, E, J, H, N, P, d, **f32)
            # element offset of (agent, env, step start + h, entity 0, feature 0) from the first element of the history view: host
            # arithmetic, so the bound on what iplan_predict will read is checked here
            s_net, s_b, s_step, s_ent, _ = src0.stride()
            row_off = (torch.arange(nA)[:, None, None] * s_net + torch.arange(E)[None, :, None] * s_b +
                       (start + torch.arange(H))[None, None, :] * s_step).to(torch.int64)
            assert int(row_off.max()) + (N - 1) * s_ent + d <= ops._room(src0)
            row_off = row_off.to(dev)
        for e0 in range(0, E, ec):
            e1 = min(E, e0 + ec)
            nz = self._noise(noise, deterministic, nA, e0, e1, (H, N, N - 1, 2), zeros=False)
            base = res["latent"][:, e0:e1]
            s0, s1 = src0[:, e0:e1], None if lat is None else lat[:, e0:e1]
            hc = None if h0 is None else h0[:, e0:e1]
            ops.gat_trace(self.gat_arena, s0[:, :, start:start + H], None if s1 is None else s1[:, :, start:start + H], hc, nz, tau=tau,
                          want=("latent",), out={"latent": base})                  # attention_trace's launch and bits
            if forecast:
                nb = e1 - e0
                pb = ops.predict(self.dec_arena, src0, row_off[:, e0:e1].reshape(nA, nb * H).contiguous(), s_ent, 0,
                                 base.reshape(nA, nb * H * N, A).contiguous(), N, P, d, checked=True)["pred"]      # predict()'s launch and bits
                pb = pb.view(nA, nb, H, N, P, d)
                res["pred"][:, e0:e1] = pb
                if keep_err:
                    # the base error in the knocked error's arithmetic: the same kernel on the base walk's latents as its one job
                    ops.predict_knockout(self.dec_arena, s0, base.unsqueeze(2), start, P, pos=pos, want=("ferr_sq",),
                                         out={"ferr_sq": res["ferr_base_sq"][:, e0:e1]})
            for j0 in range(0, J, jc):
                j1 = min(J, j0 + jc)
                out = {}
                if keep_shift:
                    out["shift_sq"] = res["shift_sq"][:, e0:e1, j0:j1]
                if keep_lat:
                    out["latent_ko"] = res["latent_ko"][:, e0:e1, j0:j1]
                elif forecast:
                    out["latent_ko"] = torch.empty(nA, e1 - e0, j1 - j0, H, N, A, **f32)      # the chunk's workspace
                if keep_attn:
                    out["attn_ko"] = res["attention_ko"][:, e0:e1, j0:j1]
                ops.gat_knockout_trace(self.gat_arena, s0, s1, hc, jobs[j0:j1], start=start, duration=D, horizon=H,
                                       base=base if keep_shift else None, noise=nz, tau=tau, knock=knock, baseline=rows, want=tuple(out), out=out)
                if forecast:
                    fout = {"fshift_sq": res["fshift_sq"][:, e0:e1, j0:j1]}
                    if keep_err:
                        fout["ferr_sq"] = res["ferr_sq"][:, e0:e1, j0:j1]
                    if keep_pk:
                        fout["pred_ko"] = res["pred_ko"][:, e0:e1, j0:j1]
                    ops.predict_knockout(self.dec_arena, s0, out["latent_ko"], start, P, pred_base=pb, pos=pos, want=tuple(fout), out=fout)
        final = {"latent": res["latent"].permute(1, 2, 0, 3, 4)}                   # [nA, E, H, ..] -> [E, H, nA, ..]
        jn = np.asarray(jobs, dtype=np.int64)
        if keep_shift:
            shift = res["shift_sq"].sqrt()                                         # [nA, E, J, H, N]
            final["latent_shift"] = shift.permute(1, 3, 0, 4, 2)
        if keep_lat:
            final["latent_ko"] = res["latent_ko"].permute(1, 3, 0, 2, 4, 5)
        if keep_attn:
            final["attention_ko"] = res["attention_ko"].permute(1, 3, 0, 2, 4, 5)
        if forecast:
            summaries = self._forecast_knockout_results(res, final, src0, jn, start, D, H, P, presence_col, keep_shift, keep_err, keep_pk,
                                                        shift if keep_shift else None)
        elif keep_shift:
            # the two means per agent and step: float64 sums and counts per (agent, env, step) formed where the shifts lie (J N times
            # fewer numbers to read back than the shifts), ONE host read-back, the environments added on the host
            win = src0[:, :, start:start + H]
            present = (win[..., presence_col] != 0) if presence_col >= 0 else torch.ones(nA, E, H, N, dtype=torch.bool, device=dev)
            jt = torch.as_tensor(jn, device=dev)
            seen = present[:, :, :D].any(dim=2)[:, :, jt]                              # [nA, E, J]: entity j present in a knocked step
            own = jt[:, None] == torch.arange(N, device=dev)[None, :]                  # [J, N]: slot j knocks ego i itself
            count = present[:, :, None] & seen[:, :, :, None, None]                    # [nA, E, J, H, N]
            parts = []
            for pick in (~own, own):
                m = count & pick[None, None, :, None, :]
                parts += [torch.where(m, shift, 0.0).sum(dim=(2, 4), dtype=torch.float64), m.sum(dim=(2, 4), dtype=torch.float64)]
            host = torch.stack(parts).cpu().numpy()                                    # [4, nA, E, H]
            tot = np.zeros((4, nA, H))
            for e in range(E):                                                         # environment order, whatever the chunks were
                tot += host[:, :, e]
            with np.errstate(divide="ignore", invalid="ignore"):
                summary = np.stack([np.where(tot[c + 1] > 0, tot[c] / tot[c + 1], np.nan) for c in (0, 2)], axis=-1)
        final = {k: (v.cpu().numpy() if as_np else v) for k, v in final.items()}
        final["knocked"] = jn
        final["sources"] = sources
        final["window"] = (start, D, H)
        if forecast:
            final.update(summaries)
        elif keep_shift:
            final["summary"] = summary
        return final

    def _forecast_knockout_results(self, res, final, src0, jn, start, D, H, P, presence_col, keep_shift, keep_err, keep_pk, shift):
        """``attention_knockout_trace(forecast=True)``: the forecast tensors of ``res`` (agent-major, sums of squares) entered into
        ``final`` in the caller's layout, and every summary of the call after ONE read-back -> dict of host arrays.  ``shift``: the
        latent shifts [nA,E,J,H,N] where ``summary`` is wanted too."""
        dev = self.device
        nA, E, S, N, _ = src0.shape
        fsh = res["fshift_sq"].sqrt()                                              # [nA, E, J, H, N, P]
        final["pred"] = res["pred"].permute(1, 2, 0, 3, 4, 5)
        final["forecast_shift"] = fsh.permute(1, 3, 0, 4, 2, 5)
        if keep_err:
            err_b = res["ferr_base_sq"].sqrt()[:, :, 0]                            # [nA, E, H, N, P]
            err_k = res["ferr_sq"].sqrt()
            final["forecast_error"] = err_b.permute(1, 2, 0, 3, 4)
            final["forecast_error_ko"] = err_k.permute(1, 3, 0, 4, 2, 5)
        if keep_pk:
            final["pred_ko"] = res["pred_ko"].permute(1, 3, 0, 2, 4, 5, 6)
        # summary's rule: a pair counts at step h when ego i is present at step start + h and entity j in at least one knocked step
        there = (src0[..., presence_col] != 0) if presence_col >= 0 else torch.ones(nA, E, S, N, dtype=torch.bool, device=dev)
        present = there[:, :, start:start + H]
        jt = torch.as_tensor(jn, device=dev)
        seen = present[:, :, :D].any(dim=2)[:, :, jt]                              # [nA, E, J]
        own = jt[:, None] == torch.arange(N, device=dev)[None, :]                  # [J, N]: slot j knocks ego i itself
        count = present[:, :, None] & seen[:, :, :, None, None]                    # [nA, E, J, H, N]
        f64 = torch.float64
        parts = []                                                                 # float64 [nA, E, H, P] each
        for pick in (~own, own):
            m = count & pick[None, None, :, None, :]
            if keep_shift:
                parts += [torch.where(m, shift, 0.0).sum(dim=(2, 4), dtype=f64)[..., None].expand(nA, E, H, P),
                          m.sum(dim=(2, 4), dtype=f64)[..., None].expand(nA, E, H, P)]
            parts += [torch.where(m[..., None], fsh, 0.0).sum(dim=(2, 4), dtype=f64), m.sum(dim=(2, 4), dtype=f64)[..., None].expand(nA, E, H, P)]
        valid = (start + np.arange(H)[:, None] + 1 + np.arange(P)[None, :]) < S    # [H, P]: the target step is recorded
        if keep_err:
            step = torch.as_tensor(np.minimum(start + np.arange(H)[:, None] + 1 + np.arange(P)[None, :], S - 1), device=dev)      # [H, P]
            target = there[:, :, step] & torch.as_tensor(valid, device=dev)[None, None, :, :, None]      # [nA, E, H, P, N]
            m = (count & ~own[None, None, :, None, :])[..., None] & target.permute(0, 1, 2, 4, 3)[:, :, None]      # [nA, E, J, H, N, P]
            parts += [torch.where(m, err_b[:, :, None], 0.0).sum(dim=(2, 4), dtype=f64), torch.where(m, err_k, 0.0).sum(dim=(2, 4), dtype=f64),
                      m.sum(dim=(2, 4), dtype=f64)]
        host = torch.stack(parts).cpu().numpy()                                    # [n, nA, E, H, P]: the ONE read-back
        tot = np.zeros((len(parts), nA, H, P))
        for e in range(E):                                                         # environment order, whatever the chunks were
            tot += host[:, :, e]
        out = {}
        k = 0
        with np.errstate(divide="ignore", invalid="ignore"):
            if keep_shift:
                out["summary"] = np.stack([np.where(tot[c + 1] > 0, tot[c] / tot[c + 1], np.nan) for c in (0, 4)], axis=-1)[:, :, 0]
                k = 2
            a, b = (k, 2 * k + 2)
            out["forecast_summary"] = np.stack([np.where(tot[c + 1] > 0, tot[c] / tot[c + 1], np.nan) for c in (a, b)], axis=-1)
            if keep_err:
                c = len(parts) - 3
                out["forecast_error_summary"] = np.stack([np.where(tot[c + 2] > 0, tot[c + i] / tot[c + 2], np.nan) for i in (0, 1)], axis=-1)
                out["forecast_valid"] = valid
        return out

    # ---------------------------------------------------------------------------- prediction saliency
    def prediction_saliency(self, history_single, attention_hidden, behavior_latent=None, columns=(1, 2), horizons=None, target=None,
                            noise=None, deterministic=True, social=None, gate="through", want=("summary",), presence_col=0,
                            max_workspace_mb=256):
        """What does the forecast of entity i at horizon step p depend on?  Inputs as ``predict``: history_single [E,nA,N,d],
        attention_hidden [E,nA,N,A], behavior_latent [E,nA,N,Z] (needed with ``GAT_use_behavior``, ignored without).  The decoder
        starts from the entity's own state x0 = history_single[.., i, :] and from the attention latent h0 = GAT(...)[i], the social
        context; for every job (horizon step p, cotangent v on the prediction y_p) ``iplan_pdec_saliency`` returns d <v, y_p> / d x0
        and d <v, y_p> / d h0 by BPTT through the autoregressive chain.
        ``columns``: the output columns whose Jacobian rows are wanted (default: highway's position columns); ``horizons``: None =
        all ``pred_length`` steps, an int, or a sorted list of distinct ints in [0, P).  ``target=None``: one one-hot job per
        (horizon, column), horizon-major; a float tensor [E,nA,N,P,d]: one job per horizon with the row ``target[.., p, :]`` as
        cotangent (``columns`` is ignored, the column axis has length 1).  ``deterministic=True`` runs the GAT without gumbel noise
        (the gate is sigmoid((l1 - l0) / tau), as ``attention_map`` / ``attention_saliency`` do it) and draws nothing; otherwise
        ``noise`` [nA,E,N,N-1,2] is used, or drawn from torch's generator as ``predict`` does.
        Returns a dict, H = len(horizons), C = len(columns):
          ``pred`` [E,nA,N,P,d]               the predictions, bit for bit ``predict``'s on the same noise
          ``latent`` [E,nA,N,A]               h0, bit for bit ``GAT_latent_update``'s
          ``state_l1``, ``latent_l1``, ``state_gxi``, ``latent_gxi`` [E,nA,N,H,C]   sum |G| and sum G x input over the columns of x0 / h0
                                              ("summary" in ``want``)
          ``state_grad`` [E,nA,N,H,C,d], ``latent_grad`` [E,nA,N,H,C,A]             the gradients ("grad" in ``want``)
          ``horizon_l1`` float64 numpy [nA,H,2]   mean of (state_l1, latent_l1) over the present rows (column ``presence_col`` of x0
                                              non-zero; < 0: every row) and over the columns -- own state against social context, per
                                              horizon; NaN where nothing counts
          ``active`` [E,nA,N,P,32] bool       the ReLU branches of the decoder's input layer ("act" in ``want``; tests)
        ``social=(p, c)`` (p in ``horizons``, c in ``columns``; with a tensor ``target``: ``social=p``) continues that one job through
        the GAT: the training-form GAT forward and ``iplan_gat_saliency`` with v_i = latent_grad[i, p, c, :] and the given ``gate``
        ("through": exact, 1/tau included; "held": the gumbel gate is a constant), in ``attention_saliency``'s chunks under
        ``max_workspace_mb`` (a row's bits do not depend on the chunking).  Adds ``pair_gl1``, ``pair_gxi`` [E,nA,N,N,n_src] (indexed
        [ego i, entity j]) and ``input_grad`` [E,nA,N,d+Z]: the GAT path summed over the egos plus, on the history columns, the direct
        path state_grad[j, p, c, :] of each entity's own row -- d sum_i y_{i,p,c} / d [history || behavior_latent]; hand its latent
        columns to ``Behavior_policy.latent_saliency`` to reach the raw history.
        numpy in -> numpy out, device tensors in -> device tensors out.  Parameters, gradients, optimiser state and (with
        ``deterministic=True``) torch's generator are not touched.  Not covered: the teacher-forced and dropout forms of the decoder
        (training only), second-order quantities, aggregation across data-parallel ranks."""
        who = "prediction_saliency"
        as_np = isinstance(history_single, np.ndarray)
        dev = self.device
        hist = _as_dev(history_single, dev)
        if hist.dim() != 4:
            raise ValueError(f"{who}: history_single must be [E,nA,N,d], got {tuple(hist.shape)}")
        E, nA, N, d = hist.shape
        A, P = self.args.attention_dim, self.pred_length
        if nA != self.n_agents or d != self.obs_shape or not 2 <= N <= ops.L.GAT_MAX_ENTITIES:
            raise ValueError(f"{who}: history_single {tuple(hist.shape)} does not fit n_agents={self.n_agents}, obs width {self.obs_shape}, "
                             f"2 <= N <= {ops.L.GAT_MAX_ENTITIES}")
        if P > ops.L.PDEC_SAL_MAX_P:
            raise NotImplementedError(f"{who}: pred_length={P} exceeds IPLAN_PDEC_SAL_MAX_P={ops.L.PDEC_SAL_MAX_P}")
        hid = _as_dev(attention_hidden, dev)
        if hid.shape != (E, nA, N, A):
            raise ValueError(f"{who}: attention_hidden {tuple(hid.shape)} != {(E, nA, N, A)}")
        if gate not in ("through", "held"):
            raise ValueError(f"{who}: gate={gate!r} is neither 'through' nor 'held'")
        want = tuple(want)
        if any(k not in ("summary", "grad", "act") for k in want):
            raise ValueError(f"{who}: want={want} -- known: 'summary', 'grad', 'act'")
        if deterministic and noise is not None:
            raise ValueError(f"{who}: noise was given together with deterministic=True")
        if not isinstance(presence_col, (int, np.integer)) or presence_col >= d:
            raise ValueError(f"{who}: presence_col={presence_col!r} outside the {d} columns")
        Z = self.args.latent_dim if self.args.GAT_use_behavior else 0
        lat = self._beh_latent(who, behavior_latent, (E, nA, N, Z))
        if lat is not None:
            lat = lat.permute(1, 0, 2, 3).contiguous()
        if noise is not None:
            noise = _as_dev(noise, dev)
            if noise.shape != (nA, E, N, N - 1, 2):
                raise ValueError(f"{who}: noise {tuple(noise.shape)} != {(nA, E, N, N - 1, 2)}")
            noise = noise.contiguous()

        def ints(x, hi, what):
            if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
                x = [x]
            try:
                x = list(x)
            except TypeError:
                raise ValueError(f"{who}: {what}={x!r} -- an int or a list of ints") from None
            if not x or any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < hi for i in x):
                raise ValueError(f"{who}: {what}={x} -- ints in [0, {hi}), at least one")
            return [int(i) for i in x]
        hz = list(range(P)) if horizons is None else ints(horizons, P, "horizons")
        if any(b <= a_ for a_, b in zip(hz, hz[1:])):
            raise ValueError(f"{who}: horizons={hz} must be sorted and distinct")
        vt = None
        if target is None:
            cols = ints(columns, d, "columns")
            if len(set(cols)) != len(cols):
                raise ValueError(f"{who}: columns={cols} must be distinct")
            jobs = [(p, c) for p in hz for c in cols]
        elif isinstance(target, (np.ndarray, torch.Tensor)) and target.ndim == 5:
            vt = _as_dev(target, dev)
            if vt.shape != (E, nA, N, P, d):
                raise ValueError(f"{who}: target {tuple(vt.shape)} != {(E, nA, N, P, d)}")
            vt = vt.permute(1, 0, 2, 3, 4).reshape(nA, E * N, P, d).contiguous()
            cols = [None]
            jobs = [(p, None) for p in hz]
        else:
            raise ValueError(f"{who}: target={target!r} -- None or a tensor [E,nA,N,P,d]")
        H, C = len(hz), len(cols)
        ks = None
        if social is not None:
            if vt is None:
                ok = isinstance(social, (tuple, list)) and len(social) == 2 and all(isinstance(i, (int, np.integer)) for i in social)
                if not ok or social[0] not in hz or social[1] not in cols:
                    raise ValueError(f"{who}: social={social!r} -- a pair (p, c) with p in horizons={hz} and c in columns={cols}")
                ks = hz.index(social[0]) * C + cols.index(social[1])
            else:
                if not isinstance(social, (int, np.integer)) or isinstance(social, bool) or social not in hz:
                    raise ValueError(f"{who}: social={social!r} -- with a tensor target, one of horizons={hz}")
                ks = hz.index(social)
            through = gate == "through"
            chunk = self._gat_saliency_chunk(who, N, through, max_workspace_mb)
        f32 = dict(dtype=torch.float32, device=dev)
        if hist.stride(3) != 1:
            hist = hist.contiguous()
        src0, hprev = hist.permute(1, 0, 2, 3), hid.permute(1, 0, 2, 3)
        nz = self._noise(noise, deterministic, nA, 0, E, (N, N - 1, 2))
        h0, _ = ops.gat_forward(self.gat_arena, src0, lat, hprev, nz)              # predict()'s launch: the rollout's bits
        grads = "grad" in want or ks is not None
        names = ("state_l1", "latent_l1", "pred") + (("state_gxi", "latent_gxi") if "summary" in want else ()) \
            + (("state_grad", "latent_grad") if grads else ()) + (("active",) if "act" in want else ())
        got = ops.pdec_saliency(self.dec_arena, hist, self._start_offsets(hist), hist.stride(2), h0.reshape(nA, E * N, A), N, P, d, jobs, v=vt,
                                want=names, checked=True)

        def rows(t, *inner):                                                       # [nA, E*N, ...] -> [E, nA, N, ...]
            return t.view(nA, E, N, *inner).permute(1, 0, 2, *range(3, 3 + len(inner)))
        res = {"pred": rows(got["pred"], P, d), "latent": h0.permute(1, 0, 2, 3)}
        per_job = {k: rows(got[k], H, C, *((d,) if k == "state_grad" else (A,) if k == "latent_grad" else ()))
                   for k in names if k not in ("pred", "active")}
        if "summary" in want:
            res.update({k: per_job[k] for k in ("state_l1", "state_gxi", "latent_l1", "latent_gxi")})
        if "grad" in want:
            res.update(state_grad=per_job["state_grad"], latent_grad=per_job["latent_grad"])
        if "act" in want:
            bit = torch.arange(32, device=dev, dtype=torch.int32)
            res["active"] = rows(((got["active"].unsqueeze(-1) >> bit) & 1).bool(), P, 32)
        if ks is not None:
            n_src, D = (2 if Z else 1), d + Z
            pair_gl1, pair_gxi = torch.empty(nA, E, N, N, n_src, **f32), torch.empty(nA, E, N, N, n_src, **f32)
            ig = torch.empty(nA, E, N, D, **f32)
            v_gat = got["latent_grad"][:, :, ks].contiguous().view(nA, E, N, A)
            self._gat_saliency_chunks(chunk, src0, lat, hprev, nz, False, 0.01, v_gat, through,
                                      dict(pair_gl1=pair_gl1, pair_gxi=pair_gxi, input_grad=ig))
            ig[..., :d] += got["state_grad"][:, :, ks].view(nA, E, N, d)           # the direct path: each entity's own start state
            res.update(pair_gl1=pair_gl1.permute(1, 0, 2, 3, 4), pair_gxi=pair_gxi.permute(1, 0, 2, 3, 4), input_grad=ig.permute(1, 0, 2, 3))
        # own state against social context, per horizon: ONE host read-back
        both = torch.stack([per_job["state_l1"], per_job["latent_l1"]], -1).cpu().numpy().astype(np.float64)      # [E, nA, N, H, C, 2]
        present = (hist[..., presence_col] != 0).cpu().numpy() if presence_col >= 0 else np.ones((E, nA, N), dtype=bool)
        count = present.sum(axis=(0, 2)).astype(np.float64) * C                   # [nA]
        sums = np.where(present[:, :, :, None, None, None], both, 0.0).sum(axis=(0, 2, 4))      # [nA, H, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            horizon_l1 = np.where(count[:, None, None] > 0, sums / count[:, None, None], np.nan)
        res = {k: (t.cpu().numpy() if as_np else t) for k, t in res.items()}
        res["horizon_l1"] = horizon_l1
        return res

    # ---------------------------------------------------------------------------- learning
    def _sample(self, n_thread, avail_len):
        """The host-side random draws of one agent in the reference's order: the (episode, t) sample of
        prediction_batch_wrapper (nova/prediction_policy.py:146) and the per-step teacher-forcing coin
        of Prediction_Decoder.forward (nova/prediction_net.py:56; drawn even at ratio 0)."""
        sel = np.random.choice(n_thread * avail_len, size=self.prediction_batch_size, replace=False)
        coins = [np.random.random() < self.args.teacher_forcing_ratio for _ in range(self.pred_length)]
        return sel, coins

    def prediction_batch_wrapper(self, history, attention_rnn, mask, behavior_latent=None):
        """nova/prediction_policy.py:122-164, vectorised: sample ``pred_batch_size`` (episode, t) pairs of one agent's
        episodes (same ``np.random.choice`` draw as the reference) and gather the input state, the stored attention /
        behaviour latents, the next ``pred_length`` states and the mask.  history [E,T,N,d], attention_rnn [E,T,N,A],
        mask [E,T], behavior_latent [E,T,N,Z] -> (input_traj [S,N,1,d], input_attention [S,N,1,A], input_latent [S,N,1,Z] or
        None, actual_traj [S,N,P,d], mask_over_traj [S,N,P,d]).  ``learn`` gathers for all agents at once instead."""
        history, attention_rnn, mask = torch.as_tensor(history), torch.as_tensor(attention_rnn), torch.as_tensor(mask)
        E, T, N, d = history.shape
        S, P = self.prediction_batch_size, self.pred_length
        avail_len = T - P - 1
        sel = torch.as_tensor(np.random.choice(E * avail_len, size=S, replace=False), dtype=torch.long, device=history.device)
        bi, ti = sel // avail_len, sel % avail_len
        input_traj = history[bi, ti].unsqueeze(2)
        input_attention = attention_rnn[bi, ti].unsqueeze(2)
        input_latent = torch.as_tensor(behavior_latent)[bi, ti].unsqueeze(2) if self.args.GAT_use_behavior else None
        steps = ti[:, None] + 1 + torch.arange(P, device=history.device)[None, :]
        actual_traj = history[bi[:, None], steps].permute(0, 2, 1, 3)
        mask_over_traj = mask[bi, ti].to(history.dtype)[:, None, None, None].expand(S, N, P, d).contiguous()
        return input_traj, input_attention, input_latent, actual_traj, mask_over_traj

    def learn(self, batch, t_env, noise=None, keep=None, defer=False, sel=None):
        """nova/prediction_policy.py:168-253 for all agents at once: sample -> fused GAT forward ->
        decoder forward + masked L1 -> decoder backward -> GAT backward -> weight gradients ->
        separate clip of the GAT and decoder groups -> Adam.  ``noise`` (gumbel, [nA, S, N, N-1, 2]) and
        ``keep`` (dropout keep flags, [nA, P, S*N, A]) may be injected; by default they are drawn from
        torch's generator on the device.  Returns the list of n_agents losses (numpy scalars); with ``defer=True``
        everything is enqueued on the current stream and a ``finish()`` callable is returned instead (it does the
        single host read-back and the logging), so independent learners can overlap on separate streams."""
        a = self.args
        dev = self.device
        nA, N, S, P = self.n_agents, self.max_vehicle_num, self.prediction_batch_size, self.pred_length
        history = batch["history"][:, :-1].to(device=dev, dtype=torch.float32)
        attention = batch["attention_latent"][:, :-1].to(device=dev, dtype=torch.float32)
        latent = batch["behavior_latent"][:, :-1].to(device=dev, dtype=torch.float32)
        term = batch["terminated"][:, :-1].to(dev)
        E, T = history.shape[:2]
        d = history.shape[-1]
        avail_len = T - P - 1
        sels, coins = zip(*[self._sample(E, avail_len) for _ in range(nA)])
        if sel is None:
            sel = torch.as_tensor(np.stack(sels), dtype=torch.long, device=dev)    # [nA, S]
        else:                                                                       # injected (episode * avail_len + t) indices
            sel = torch.as_tensor(np.asarray(sel), dtype=torch.long, device=dev)
            S = sel.shape[1]
        bi, ti = sel // avail_len, sel % avail_len
        ag = torch.arange(nA, device=dev)[:, None].expand(nA, S)
        # gathers = data movement only (prediction_batch_wrapper, :123-164)
        x0 = history[bi, ti, ag].contiguous()                                      # [nA, S, N, d]
        att = attention[bi, ti, ag].contiguous()                                   # [nA, S, N, A]
        lat = latent[bi, ti, ag].contiguous() if a.GAT_use_behavior else None
        steps = ti[:, :, None] + 1 + torch.arange(P, device=dev)[None, None, :]
        actual = history[bi[:, :, None], steps, ag[:, :, None]].permute(0, 1, 3, 2, 4).contiguous()   # [nA, S, N, P, d]
        mask = term[bi, ti, ag, 0].to(torch.float32).contiguous()                  # [nA, S]  (polarity as the reference: :191)
        if noise is None:
            noise = gumbel_noise((nA, S, N, N - 1, 2), dev)
        if keep is None and a.decoder_dropout > 0:
            keep = torch.empty(nA, P, S * N, a.attention_dim, device=dev).bernoulli_(1.0 - a.decoder_dropout)
        teacher = None
        if any(any(c) for c in coins):
            teacher = torch.as_tensor(np.array(coins, dtype=np.int32), device=dev).contiguous()
        hid, saved = ops.gat_forward(self.gat_arena, x0, lat, att, noise, save=True)
        # data-parallel runs: the loss normaliser counts the samples of ALL ranks (parallel.py)
        dp = getattr(self, "dp", None)
        mask_sum = dp.all_reduce_sum(mask.sum(dim=1)) if dp is not None else None
        fwd = ops.pdec_forward(self.dec_arena, x0.reshape(nA, S * N, d), hid.reshape(nA, S * N, -1),
                               actual.reshape(nA, S * N, P, d), mask, N, keep=keep, drop_p=a.decoder_dropout, teacher=teacher,
                               mask_sum=mask_sum)
        g_h0 = ops.pdec_backward(self.dec_arena, fwd)
        ops.gat_backward(self.gat_arena, saved, g_h0.reshape(nA, S, N, -1))
        if getattr(self, "dp", None) is not None:
            self.dp.all_reduce_grads(self.gat_arena, self.dec_arena)
        sq = step_all(self.pred_optimizer, self.max_grad_norm if self._use_max_grad_norm else None)
        stats = torch.cat([fwd["loss"], sq.sqrt().reshape(-1)])
        staged = AsyncHost(stats) if defer else None             # deferred: staged behind THIS stream's work, read whenever

        def finish():
            host = staged.get() if staged is not None else stats.cpu()              # ONE host read-back
            losses = host[:nA].numpy()
            norms = host[nA:].reshape(nA, 2)
            train_info = {"prediction_loss": float(losses.sum()), "pred_encoder_grad_norm": float(norms[:, 0].sum()),
                          "pred_decoder_grad_norm": float(norms[:, 1].sum())}
            if t_env - self.log_stats_t >= self.args.learner_log_interval:
                for k, v in train_info.items():
                    self.logger.log_stat(self.log_prefix + k, v, t_env)
            return [np.asarray(x) for x in losses]
        return finish if defer else finish()

    # ---------------------------------------------------------------------------- checkpoints
    def save_models(self, path):
        for i in range(self.n_agents):
            torch.save(self.pred_GAT[i].state_dict(), f"{path}/pred_GAT_{i}.th")
            torch.save(self.pred_decoder[i].state_dict(), f"{path}/pred_decoder_{i}.th")
            torch.save(self.pred_optimizer[i].state_dict(), f"{path}/pred_optimizer_{i}_opt.th")

    def load_models(self, paths, load_optimisers=False):
        if len(paths) == 1:
            paths = [copy.copy(paths[0]) for _ in range(self.n_agents)]
        for i in range(self.n_agents):
            self.pred_GAT[i].load_state_dict(torch.load(f"{paths[i]}/pred_GAT_{i}.th", map_location="cpu"))
            self.pred_decoder[i].load_state_dict(torch.load(f"{paths[i]}/pred_decoder_{i}.th", map_location="cpu"))
            if load_optimisers:
                self.pred_optimizer[i].load_state_dict(
                    torch.load(f"{paths[i]}/pred_optimizer_{i}_opt.th", map_location="cpu"))
