"""Behavior_policy (soft update = iPLAN) -- behavioural-incentive inference module (mirror of
nova/stable_behavior_policy.py:13-312)."""
import copy
import contextlib
import os

import numpy as np
import torch

from .. import ops
from ..arena import ParamArena
from ..optim import FusedAdam, step_all
from ..streams import AsyncHost, distinct_stream, masked_stream, probe_mode
from .behavior_net import Behavior_Latent_Decoder, EncoderRNN
from .prediction_policy import _as_dev

EPS = 1e-10


def _history_dims(who, entry, policy, history):
    """``history`` [E, T, nA, N, d] (numpy or tensor) fits ``policy`` and ``entry``'s window limit -> (as_np, E, T, nA, N, d, J)"""
    as_np = isinstance(history, np.ndarray)
    if not as_np and not torch.is_tensor(history):
        raise ValueError(f"{who}: history must be a numpy array or a tensor [E, T, nA, N, d]")
    if history.ndim != 5:
        raise ValueError(f"{who}: history must be [E, T, nA, N, d], got {tuple(history.shape)}")
    E, T, nA, N, d = (int(s) for s in history.shape)
    Lw = policy.max_history_len
    J = T - 1 - Lw
    if nA != policy.n_agents or d != policy.args.obs_shape_single or E < 1 or N < 1:
        raise ValueError(f"{who}: history {tuple(history.shape)} does not fit n_agents={policy.n_agents}, d={policy.args.obs_shape_single}")
    if J < 1:
        raise ValueError(f"{who}: T={T} leaves no window (J = T - 1 - L = {J})")
    if Lw > ops.L.ENC_SAL_MAX_L:
        raise NotImplementedError(f"{who}: max_history_len={Lw} > {ops.L.ENC_SAL_MAX_L} is not supported by {entry}")
    return as_np, E, T, nA, N, d, J


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _as_int(who, v, what):
    if not _is_int(v):
        raise ValueError(f"{who}: {what} must be an int, got {v!r}")
    return int(v)


def _int_list(who, v, what, entry, kinds="an int or a sequence of ints", text=False):
    """an int or a sequence of ints -> list; ``entry`` names an element and ``kinds`` what is accepted in the messages; ``text``: a str is
    taken as a sequence (and refused character by character), not refused as a whole"""
    if _is_int(v):
        return [int(v)]
    if not text and isinstance(v, (str, bytes)):
        raise ValueError(f"{who}: {what} must be {kinds}, got {v!r}")
    try:
        return [_as_int(who, j, entry) for j in list(v)]
    except TypeError:
        raise ValueError(f"{who}: {what} must be {kinds}, got {v!r}") from None


def _sorted_inside(who, idx, what, J):
    if not idx or any(j < 0 or j >= J for j in idx) or any(b <= a for a, b in zip(idx, idx[1:])):
        raise ValueError(f"{who}: {what} must be sorted, distinct and inside [0, J={J}), got {idx}")


def _net_major(h, d):
    """[E, T, nA, N, d] -> the [nA, E, T, N, d] view the encoder ops read in place (a copy where the (N, d) rows are not contiguous)"""
    hist = h.permute(2, 0, 1, 3, 4)
    return hist if hist.stride(4) == 1 and hist.stride(3) == d else hist.contiguous()


def _chunks(who, E, n, shared, each, max_workspace_mb, item):
    """Envs first; where ONE env with all ``n`` items does not fit under ``max_workspace_mb``, groups of items as well.  ``shared``:
    floats per env whatever the number of items, ``each``: floats per env and item -> (envs per chunk, [(first, end) of every group])"""
    limit = int(max_workspace_mb * 2 ** 20) // 4
    per_env = shared + n * each
    if per_env <= limit:
        return min(E, limit // per_env), [(0, n)]
    g = (limit - shared) // each
    if g < 1:
        raise ValueError(f"{who}: max_workspace_mb={max_workspace_mb} is too small for one env and one {item} ({4 * (shared + each)} bytes)")
    return 1, [(i, min(n, i + g)) for i in range(0, n, g)]


def _to_numpy(res):
    """a dict of device tensors as host arrays of the matching dtypes, by ONE read-back (every piece is exactly representable in float64)"""
    keys = list(res)
    host = torch.cat([res[k].reshape(-1).double() for k in keys]).cpu().numpy()
    out_np, at = {}, 0
    for k in keys:
        n = res[k].numel()
        piece = host[at:at + n].reshape(tuple(res[k].shape))
        at += n
        out_np[k] = piece.astype({torch.float32: np.float32, torch.int64: np.int64, torch.bool: np.bool_}.get(res[k].dtype, np.float64))
    return out_np


class Behavior_policy:
    def __init__(self, args, logger):
        self.device = torch.device("cuda" if args.use_cuda else "cpu")
        self.args = args
        self.n_actions = args.n_actions
        self.n_agents = args.n_agents
        self.max_vehicle_num = args.max_vehicle_num
        self.max_history_len = args.max_history_len
        self.latent_dim = args.latent_dim
        self.optim_eps = args.optim_eps
        self.weight_decay = args.weight_decay
        self.obs_shape = args.obs_shape
        self.init_behavior_net()
        self.logger = logger
        self.log_prefix = args.log_prefix
        self.log_stats_t = -self.args.learner_log_interval - 1
        self._use_max_grad_norm = args.use_max_grad_norm
        self.max_grad_norm = args.max_grad_norm
        self.soft_update_coef = args.soft_update_coef
        self.behavior_variation_penalty = args.behavior_variation_penalty
        self.thres_small_variation = args.thres_small_variation

    def init_behavior_net(self):
        """nova/stable_behavior_policy.py:56-80."""
        a = self.args
        self.behavior_encoder, self.behavior_decoder = [], []
        for _ in range(self.n_agents):
            self.behavior_encoder.append(EncoderRNN(input_size=a.obs_shape_single, hidden_size=a.encoder_rnn_dim,
                                                    output_size=a.latent_dim, num_layers=a.num_encoder_layer))
            self.behavior_decoder.append(Behavior_Latent_Decoder(
                input_size=a.obs_shape_single + a.latent_dim, hidden_size=a.decoder_rnn_dim,
                output_size=a.obs_shape_single, num_layers=a.num_decoder_layer, dropout=a.decoder_dropout))
        self.enc_arena = ParamArena(self.behavior_encoder, self.device)
        self.dec_arena = ParamArena(self.behavior_decoder, self.device)
        for i in range(self.n_agents):
            self.behavior_encoder[i].attach(self.enc_arena, i)
            self.behavior_decoder[i].attach(self.dec_arena, i)
        self.behavior_optimizer = [
            FusedAdam([(self.enc_arena, i), (self.dec_arena, i)], lr=a.lr_behavior, eps=self.optim_eps,
                      weight_decay=self.weight_decay) for i in range(self.n_agents)]

    # ---------------------------------------------------------------------------- rollout
    def latent_update(self, history, encoder_hidden, prev_latent, out_latent=None, out_hidden=None, launch=True):
        """history [E,nA,N,L,d], encoder_hidden [E,layers,nA,N,R], prev_latent [E,nA,N,Z] ->
        (new_latent [E,nA,N,Z], new_hidden [E,layers,nA,N,R])  (stable_behavior_policy.py:83-123).
        numpy history -> numpy latent + torch hidden (as the reference returns); device tensors in
        -> device tensors out.  One fused launch for all agents, soft update included.  ``history`` may be any
        strided device view (a sliding window over a time-major log is read in place); ``out_latent`` [E,nA,N,Z]
        / ``out_hidden`` [E,nA,N,R]: optional destination views written by the kernel."""
        as_np = isinstance(history, np.ndarray)
        hist = _as_dev(history, self.device)
        hid = _as_dev(encoder_hidden, self.device)
        prev = _as_dev(prev_latent, self.device)
        E, nA, N, L, d = hist.shape
        res = ops.enc_forward(self.enc_arena, hist.permute(1, 0, 2, 3, 4), hid[:, 0].permute(1, 0, 2, 3),
                              prev.permute(1, 0, 2, 3), self.soft_update_coef, self.latent_dim,
                              out_lat=None if out_latent is None else out_latent.permute(1, 0, 2, 3),
                              out_h=None if out_hidden is None else out_hidden.permute(1, 0, 2, 3), launch=launch)
        if not launch:                                    # device-resident rollout: the launch is fused into the GAT's
            return res[2]                                 # (``Prediction_policy.GAT_latent_update(fuse_enc=...)``)
        lat, hL = res
        lat = lat.permute(1, 0, 2, 3)                     # [E, nA, N, Z]
        hL = hL.permute(1, 0, 2, 3).unsqueeze(1)          # [E, 1, nA, N, R]
        if as_np:
            return lat.cpu().numpy(), hL
        return lat, hL


    # ---------------------------------------------------------------------------- learning
    def behavior_traj_wrapper(self, history, step, mask):
        """nova/stable_behavior_policy.py:128-157, vectorised: window ``step`` of one agent's episode.
        history [E, T, N, d], mask [E, T] -> (curr [E,N,L,d] = steps step-L+1..step right-aligned / zero-padded,
        next [E,N,L,d] = steps step+1..step+L, and their per-step masks broadcast to the same shapes; padded positions of the
        current mask stay 1 like the reference's).  ``learn`` does not call this -- the kernels walk the windows in place --
        it is kept for callers that want the reference's per-window tensors."""
        history, mask = torch.as_tensor(history), torch.as_tensor(mask)
        E, T, N, d = history.shape
        L = self.max_history_len
        start, plug = max(0, step - L + 1), max(0, L - step - 1)
        curr = torch.zeros(E, N, L, d, dtype=history.dtype, device=history.device)
        curr[:, :, plug:] = history[:, start:step + 1].permute(0, 2, 1, 3)
        nxt = history[:, step + 1:step + L + 1].permute(0, 2, 1, 3)
        m = mask.to(history.dtype)
        m_curr = torch.ones_like(curr)
        m_curr[:, :, plug:] = m[:, start:step + 1, None, None].permute(0, 2, 1, 3).expand(E, N, step + 1 - start, d)
        m_next = m[:, step + 1:step + L + 1, None, None].permute(0, 2, 1, 3).expand(E, N, L, d).contiguous()
        return curr, nxt, m_curr, m_next

    def _global_window_sums(self, mask, hard=False):
        """The loss normalisers (mask sums per window), over ALL ranks' envs in data-parallel runs.  Always handed to the
        kernels: their in-kernel fallback re-sums E x L mask entries per window in every wave (a dependent-load loop that
        cost the decoder kernels about a tenth of their time at 110 envs)."""
        dp = getattr(self, "dp", None)
        if dp is None and os.environ.get("IPLAN_BEH_KERNEL_WINSUM"):             # (timing experiments: the in-kernel sums)
            return None
        wn = ops.beh_window_mask_sums(mask, self.max_history_len, hard=hard)
        return wn if dp is None else dp.all_reduce_sum(wn)

    def _global_envs(self, E):
        """envs the stability statistic is averaged over: this process's, times the data-parallel world size"""
        dp = getattr(self, "dp", None)
        return E * (dp.world if dp is not None else 1)

    def join_decoder(self):
        """Make the current stream wait for a decoder update that ``learn(..., defer_decoder=True)`` left running on the side
        stream (no-op otherwise).  Everything that reads or writes the decoder's parameters calls this first."""
        self.flush_decoder()
        ev = getattr(self, "_dec_done", None)
        if ev is not None and self.defer_late == 1:
            # (the update was enqueued moments ago: a host wait here would stall the enqueue of this call's own forward; the
            # allocator alternates between two sets of record blocks instead)
            torch.cuda.current_stream(self.device).wait_event(ev)
            self._dec_done = None
        elif ev is not None:
            # HOST wait, not just a stream wait: the update holds the previous call's 23 GB of BPTT records (record_stream);
            # until its event has completed the caching allocator cannot hand those blocks to this call and would go to
            # hipMalloc for fresh ones (+13 ms per call, measured)
            ev.synchronize()
            torch.cuda.current_stream(self.device).wait_event(ev)
            self._dec_done = None

    defer_late = int(os.environ.get("IPLAN_DEFER_LATE", "0"))

    def flush_decoder(self):
        """Enqueue a decoder update that ``learn(..., defer_decoder=True)`` held back (IPLAN_DEFER_LATE), behind the work the
        current stream holds now.  The training loop calls it when the next rollout has been enqueued; ``join_decoder`` calls it too."""
        f = getattr(self, "_dec_pending", None)
        if f is not None:
            self._dec_pending = None
            f()

    learn_takes_prepared = True         # (subclasses with their own ``learn`` signature switch it off)

    def prepare_learn(self, batch):
        """The data-movement head of ``learn``: episode views, the [nA, E, T] float mask (polarity as the reference's, :190-193) and the
        per-window mask sums (all ranks' in data-parallel runs).  A training loop that enqueues other learners beside ``learn`` calls
        this FIRST and passes the result as ``learn(..., prepared=)``: these few tiny launches otherwise queue behind the other
        learners' kernels at the head of the learn phase."""
        v = self._episode_views(batch)
        v["win_norm"] = self._global_window_sums(v["mask"])
        return v

    def _episode_views(self, batch):
        """``prepare_learn`` without the (possibly all-reduced) window sums: what ``evaluate`` shares with ``learn``"""
        a, dev = self.args, self.device
        history = batch["history"][:, :-1].to(device=dev, dtype=torch.float32)     # [E, T, nA, N, d]
        term = batch["terminated"][:, :-1].to(dev)                                 # [E, T, nA, 1]
        mask = (1 - term[..., 0]) if a.env == "MPE" else term[..., 0]
        mask = mask.permute(2, 0, 1).to(torch.float32).contiguous()                # [nA, E, T]
        return dict(batch=batch, history=history, mask=mask, hist=history.permute(2, 0, 1, 3, 4))   # hist: [nA, E, T, N, d] view

    def learn(self, batch, t_env, keep=None, defer_decoder=False, defer_readback=False, prepared=None):
        """nova/stable_behavior_policy.py:161-279 for all agents at once: ONE persistent forward launch
        walks every (env, entity) chain through the T-1-L windows (decoder + encoder GRUs, soft latent
        update, masked L1), ONE backward launch does the BPTT, then weight-gradient contractions,
        separate clipping of the encoder and decoder groups and Adam.  ``keep`` (uint8 dropout keep flags
        [nA, J, E*N, L, 64]) may be injected; by default the kernel draws them from a counter-based
        generator seeded from torch's RNG.  Returns (behavior_loss, stability_loss, total_loss) lists.

        ``defer_decoder=True`` (device-resident training loops): the DECODER's weight-gradient contraction, gradient
        all-reduce, clip and Adam step are enqueued on a side stream and this call returns once the encoder is updated.
        Nothing outside behaviour learning reads the decoder (the rollout uses the encoder only), so that work -- the largest
        bandwidth-bound item of a ``learn`` -- runs beside the next rollout, whose kernels leave 96 of the 256 CUs idle; the
        next ``learn`` (and save / load) waits for it.  Same arithmetic, same order of optimiser steps; the logged decoder
        gradient norm is the previous call's.

        ``defer_readback=True``: the call does not wait for the device at all -- the losses / gradient norms are staged to
        pinned host memory behind the enqueued work and the call returns a function that delivers the three lists (and logs)
        when called; the host can then enqueue the next rollout while this call's kernels still run."""
        a = self.args
        dev = self.device
        self.join_decoder()
        if prepared is None or prepared["batch"] is not batch:
            prepared = self.prepare_learn(batch)
        history, mask, hist, wn_all = prepared["history"], prepared["mask"], prepared["hist"], prepared["win_norm"]
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if keep is None else 0
        E, N = history.shape[0], self.max_vehicle_num
        chunk = int(getattr(a, "behavior_env_chunk", 0) or os.environ.get("IPLAN_BEH_ENV_CHUNK", "128"))
        if E <= chunk:
            fwd = ops.beh_forward(self.enc_arena, self.dec_arena, hist, mask, self.max_history_len, self.latent_dim,
                                  self.soft_update_coef, self.thres_small_variation, a.decoder_dropout, keep=keep, seed=seed,
                                  win_norm=wn_all)
            defer = bool(defer_decoder)
            bwd = ops.beh_backward(self.enc_arena, self.dec_arena, fwd, penalty=self.behavior_variation_penalty,
                                   E_norm=self._global_envs(E), defer_dec_wgrad=defer)
            loss_dev = fwd["loss"]
        else:
            defer = False
            if defer_decoder and not getattr(self, "_warned_chunked_defer", False):
                self._warned_chunked_defer = True
                print(f"Behavior_policy.learn: defer_decoder ignored -- {E} envs are learnt in chunks of {chunk} "
                      "(one optimiser step behind the last chunk, decoder included)")
            # Large batches (config 4's 256 envs on one GPU: 230 GB of BPTT records at once): env chunks run one after the
            # other -- chains never interact; the loss normalisers are the window mask sums over ALL envs (and ranks), so
            # the chunk gradients simply add up in the arenas -- and one clip + Adam step follows.
            wn = wn_all
            loss_dev = None
            for c, lo in enumerate(range(0, E, chunk)):
                hi = min(E, lo + chunk)
                fwd = ops.beh_forward(self.enc_arena, self.dec_arena, hist[:, lo:hi], mask[:, lo:hi].contiguous(), self.max_history_len,
                                      self.latent_dim, self.soft_update_coef, self.thres_small_variation, a.decoder_dropout,
                                      keep=None if keep is None else keep[:, :, lo * N:hi * N].contiguous(),
                                      seed=seed + 0x9E3779B97F4A7C15 * c & (2 ** 63 - 1), win_norm=wn)
                ops.beh_backward(self.enc_arena, self.dec_arena, fwd, accumulate=c > 0, penalty=self.behavior_variation_penalty,
                                 E_norm=self._global_envs(E))
                part = fwd["loss"] * torch.tensor([1.0, (hi - lo) / E], device=dev)      # the stability statistic is a mean over envs
                loss_dev = part if loss_dev is None else loss_dev + part
                del fwd
        max_norm = self.max_grad_norm if self._use_max_grad_norm else None
        nA = self.n_agents
        if E <= chunk and defer:
            # encoder now (the next rollout needs it) ...
            if getattr(self, "dp", None) is not None:
                self.dp.all_reduce_grads(self.enc_arena)
            sq = step_all(self.behavior_optimizer, max_norm, slices=(0,))
            steps = self.behavior_optimizer[0].last_steps
            prev_dec = getattr(self, "_dec_sq", None)
            # ... decoder on the side stream, same optimiser step
            on_gpu = torch.device(dev).type == "cuda"
            if on_gpu and getattr(self, "_dec_stream", None) is None:
                # plain side stream by default; IPLAN_DEFER_CUS=k restricts it to k CUs (see harness.py / profiles/r02e_notes.md)
                cus = int(os.environ.get("IPLAN_DEFER_CUS", "0"))
                # (beside the NEXT rollout: not on the caller's hardware queue, streams.distinct_stream)
                # (beside the NEXT rollout: not on the caller's hardware queue when queues are probed, streams.distinct_stream.  Sharing the
                # prediction learner's stream instead was measured: no better without RCCL, worse with it -- profiles/r06_notes.md section 8)
                self._dec_stream = masked_stream(dev, cus) if cus > 0 else (
                    distinct_stream(dev, [torch.cuda.current_stream(dev)]) if probe_mode() == "full" else torch.cuda.Stream(dev))
            ds = self._dec_stream if on_gpu else None                   # (CPU / emulator: same code, run in line)

            def update(bwd=bwd):
                bwd["dec_wgrad"](ds)                                    # (behind whatever the CALLER's stream holds at this point)
                with (torch.cuda.stream(ds) if on_gpu else contextlib.nullcontext()):
                    if getattr(self, "dp", None) is not None:
                        self.dp.all_reduce_grads(self.dec_arena)
                    # (its own norm buffer: the encoder half of the NEXT call fills the shared one on the main stream while this
                    # half may still be running here)
                    if getattr(self, "_dec_sq_buf", None) is None:
                        self._dec_sq_buf = torch.zeros(nA, len(self.behavior_optimizer[0].slices), dtype=torch.float32, device=dev)
                    sq_d = step_all(self.behavior_optimizer, max_norm, slices=(1,), steps=steps, sq=self._dec_sq_buf)
                    self._dec_sq = sq_d[:, 1].clone()
                    if on_gpu:
                        self._dec_done = torch.cuda.Event()
                        self._dec_done.record(ds)

            # IPLAN_DEFER_LATE=1 (A/B knob): the update is not enqueued here but handed to the training loop, which starts it
            # (flush_decoder) once the NEXT rollout is on the device -- the wide contraction holds every SIMD for ~2.7 ms, and
            # started here it does so in front of that rollout's first, latency-bound launches.  Same values either way.
            if on_gpu and self.defer_late:
                self._dec_pending = update
            else:
                update()
            del update
            del bwd
            dec_col = prev_dec if prev_dec is not None else torch.zeros(nA, device=dev)
            host_dev, split = torch.cat([loss_dev.reshape(-1), sq[:, 0].sqrt(), dec_col.sqrt()]), True
        else:
            if getattr(self, "dp", None) is not None:
                self.dp.all_reduce_grads(self.enc_arena, self.dec_arena)
            sq = step_all(self.behavior_optimizer, max_norm)
            host_dev, split = torch.cat([loss_dev.reshape(-1), sq.sqrt().reshape(-1)]), False
        if torch.device(dev).type == "cuda" and not getattr(self, "_queues_checked", False):
            # first learn() done: the encoder's side streams have their hardware queues -- not the caller's, or they get replaced
            # (ops.verify_side_queues; a training loop with more streams to place, harness.cycle, runs its own wider check)
            self._queues_checked = True
            if not defer_readback:
                ops.verify_side_queues(dev, torch.cuda.current_stream(dev))
        staged = AsyncHost(host_dev) if defer_readback else None

        def finish():
            host = staged.get() if staged is not None else host_dev.cpu()              # ONE host read-back
            loss = host[:2 * nA].reshape(nA, 2).numpy()
            norms = host[2 * nA:].reshape(2, nA).t() if split else host[2 * nA:].reshape(nA, 2)
            beh = [np.asarray(loss[i, 0]) for i in range(nA)]
            stab = [np.asarray(loss[i, 1]) for i in range(nA)]
            total = [np.asarray(loss[i, 0] + self.behavior_variation_penalty * loss[i, 1]) for i in range(nA)]
            train_info = {"behavior_loss": float(loss[:, 0].sum()), "stability_loss": float(loss[:, 1].sum()),
                          "behavior_total": float(sum(float(t) for t in total)),
                          "behavior_encoder_grad_norm": float(norms[:, 0].sum()),
                          # deferred decoder update: the norm of the PREVIOUS call's decoder step (this call's is still on its
                          # way; 0 on the first call) -- flagged by the extra stat below
                          "behavior_decoder_grad_norm": float(norms[:, 1].sum())}
            if split:
                train_info["behavior_decoder_grad_norm_lag_calls"] = 1.0
            if t_env - self.log_stats_t >= self.args.learner_log_interval:
                for k, v in train_info.items():
                    self.logger.log_stat(self.log_prefix + k, v, t_env)
            return beh, stab, total
        return finish if defer_readback else finish()

    # ---------------------------------------------------------------------------- inference
    def evaluate(self, batch, return_latent=False, return_reconstruction=False, defer=False):
        """How well the current encoder / decoder reconstruct an episode batch: the forward of ``learn`` run deterministically
        -- no dropout whatever ``decoder_dropout`` is, no draw from any generator -- and without touching parameters or
        optimiser state.  Same episode views and mask polarity as ``learn`` (``prepare_learn``); ONE forward-only launch for
        all agents and all envs (csrc/behavior_eval.hip: nothing is recorded for a backward pass, so there is no env
        chunking), one host read-back.  Returns a dict of host arrays (float64):
          behavior_loss, stability_loss, total_loss  [nA]: the three values ``learn`` reports, formed from the kernel's sums
              as the reference forms them (masked L1 / (sum(mask) + EPS) * d * N per window, clamped distance / E / L, mean
              over the J = T - 1 - L windows; total = behaviour + behavior_variation_penalty * stability)
          l1_per_step  [nA, L]: mean absolute error per feature at look-ahead step t over the (env, entity, window) triples
              whose mask is set; NaN where nothing counts
          count        [nA, L]: those triples
          latent         [E, J, nA, N, Z]     (``return_latent``): the intent latent after every window's update
          reconstruction [E, J, nA, N, L, d]  (``return_reconstruction``): the decoder's output for every window
        ``defer=True``: everything is enqueued on the current stream and a ``finish()`` callable is returned that does the
        read-back.  The values are THIS process's own: a data-parallel ``dp`` attachment is not consulted (every rank
        evaluates the episodes it is given)."""
        self.join_decoder()
        v = self._episode_views(batch)
        mask, hist = v["mask"], v["hist"]
        nA, E, T, N, d = hist.shape
        L_win, Z = self.max_history_len, self.latent_dim
        J = T - 1 - L_win
        out = ops.beh_eval(self.enc_arena, self.dec_arena, hist, mask, L_win, Z, self.soft_update_coef, self.thres_small_variation,
                           want_latent=return_latent, want_recon=return_reconstruction, want_sums=True)
        wn = ops.beh_window_mask_sums(mask, L_win)                                   # [nA, J]: this process's envs only
        col = mask.sum(dim=1)                                                        # [nA, T]
        steps = torch.arange(J, device=col.device)[:, None] + 1 + torch.arange(L_win, device=col.device)[None, :]
        count = col[:, steps].sum(dim=1) * N                                         # [nA, L] (sums of 0/1 flags: exact)
        pieces = [out["sums"].reshape(-1), wn.reshape(-1), count.reshape(-1)]
        if return_latent:
            pieces.append(out["latent"].reshape(-1))
        if return_reconstruction:
            pieces.append(out["recon"].reshape(-1))
        host_dev = torch.cat(pieces)
        staged = AsyncHost(host_dev) if defer else None
        penalty = self.behavior_variation_penalty

        def finish():
            host = (staged.get() if staged is not None else host_dev.cpu()).numpy()      # ONE host read-back
            at = 0

            def take(*shape):
                nonlocal at
                n = int(np.prod(shape))
                piece = host[at:at + n].reshape(shape)
                at += n
                return piece
            s = take(nA, J, L_win, 2).astype(np.float64)
            w = take(nA, J).astype(np.float64)
            cnt = take(nA, L_win).astype(np.float64)
            beh = (s[..., 0].sum(2) / (w * (N * d) + EPS) * (d * N)).sum(1) / J
            stab = (s[..., 1].sum(2) / E / L_win).sum(1) / J
            with np.errstate(divide="ignore", invalid="ignore"):
                l1 = np.where(cnt > 0, s[..., 0].sum(1) / (cnt * d), np.nan)
            res = {"behavior_loss": beh, "stability_loss": stab, "total_loss": beh + penalty * stab, "l1_per_step": l1, "count": cnt}
            if return_latent:
                res["latent"] = take(nA, E, N, J, Z).transpose(1, 3, 0, 2, 4).copy()
            if return_reconstruction:
                res["reconstruction"] = take(nA, E, N, J, L_win, d).transpose(1, 3, 0, 2, 4, 5).copy()
            return res
        return finish if defer else finish()

    def latent_trace(self, history):
        """The intent latent the encoder assigns to every vehicle after every window of an episode: history [E, T, nA, N, d]
        (the steps ``learn`` sees, i.e. already without the episode's last one) -> [E, J, nA, N, Z], J = T - 1 - L; entry j is
        the latent after the soft update of window j (steps j-L+1 .. j, zero-padded in front), from latent = 0 and a zero
        hidden state at j = 0 -- what ``latent_update`` gives when it is driven over the same windows step by step.  numpy in
        -> numpy out, device tensor in -> device tensor out.  One forward-only launch; no parameter, optimiser or generator
        state is touched, and a data-parallel ``dp`` attachment is not consulted."""
        self.join_decoder()
        as_np = isinstance(history, np.ndarray)
        h = _as_dev(history, self.device)
        E, T, nA, N, d = h.shape
        out = ops.beh_eval(self.enc_arena, self.dec_arena, h.permute(2, 0, 1, 3, 4), None, self.max_history_len, self.latent_dim,
                           self.soft_update_coef, self.thres_small_variation, want_latent=True, want_recon=False, want_sums=False)
        J = T - 1 - self.max_history_len
        lat = out["latent"].reshape(nA, E, N, J, self.latent_dim).permute(1, 3, 0, 2, 4)
        return lat.cpu().numpy() if as_np else lat

    def latent_saliency(self, history, windows=None, lags=None, target="argmax", want=("step",), presence_col=0, max_workspace_mb=256):
        """Which past steps, and which features, make the encoder assign a vehicle its intent: the derivative of the latent
        ``latent_trace`` returns with respect to the RAW history, by BPTT through the encoder chain (csrc/enc_saliency.hip).
        history [E, T, nA, N, d] as for ``latent_trace`` (numpy in -> numpy out, device tensor in -> device tensors out).
          windows  None = the last window J - 1 (J = T - 1 - L), an int, or a sorted sequence of distinct ints in [0, J); W = their number
          lags     K, the number of earlier windows that are unrolled; None = max(windows), i.e. everything.  For target window j the
                   windows j - Kj .. j, Kj = min(K, j), are differentiated and he / latent of window j - Kj - 1 are held constant (both
                   are zero when Kj = j: the result is then the exact total derivative).  R = K + L steps are reported.
          target   the cotangent v of y = <v, lat_j>: "argmax" = one-hot of the chain's own argmax_z lat_j (lowest index on ties; returned
                   as target_index), an int z = that component everywhere, or a float tensor [E, W, nA, N, Z] -- e.g. the ``beh`` columns
                   of ``DcntrlMAC.saliency(..., want=("input_grad",))``'s actor_input_grad, which continues the policy's saliency back to
                   the history
          want     any of "step", "grad", "act"
        With G[r, c] = d y / d x_{j-r, c}, returns a dict of
          step_l1, step_gxi [E, W, nA, N, R]   sum_c |G[r, c]|  and  sum_c G[r, c] x_{j-r, c}                       ("step")
          feature_l1        [E, W, nA, N, d]   sum_r |G[r, c]|                                                     ("step")
          grad              [E, W, nA, N, R, d]                                                                    ("grad")
          active            [E, W, nA, N, K+1, L] int64: bit m = unit m of the encoder's input Linear is past its ReLU at recomputed
                            window j - k, position t; 0 where that window does not exist                           ("act")
          latent            [E, W, nA, N, Z]   lat_j of the target windows
          step_valid        [W, R] bool        entries that exist: j - r >= 0 and r <= Kj + L - 1; G is exactly 0 elsewhere
          target_index      [E, W, nA, N] int64 (target="argmax")
          carry_l2          [E, W, nA, N]      || d y / d he_{j-Kj-1} ||_2, what still flows into the state beyond the truncation (0 where Kj = j)
          lag_l1            [nA, R] float64    the mean of step_l1[..., r] over the (env, window, vehicle) entries that are valid and, with
                            ``presence_col`` not None, have x_j[presence_col] != 0; 0 where nothing counts -- "how far back does the intent look"
        Envs (and, where one env does not fit, windows) are processed in chunks so that the kernel's scratch stays under
        ``max_workspace_mb``; chunked and unchunked calls give the same bits.  Deterministic; draws from no generator; no parameter,
        gradient, optimiser or carried state is touched; a data-parallel ``dp`` attachment is not consulted."""
        self.join_decoder()
        who = "latent_saliency"
        as_np, E, T, nA, N, d, J = _history_dims(who, "iplan_enc_saliency", self, history)
        Lw, Z, dev = self.max_history_len, self.latent_dim, self.device
        win = [J - 1] if windows is None else _int_list(who, windows, "windows", "a window", kinds="None, an int or a sequence of ints", text=True)
        _sorted_inside(who, win, "windows", J)
        W = len(win)
        K = max(win) if lags is None else _as_int(who, lags, "lags")
        if K < 0:
            raise ValueError(f"latent_saliency: lags={K} is negative")
        R = K + Lw
        want = (want,) if isinstance(want, str) else tuple(want)
        if any(k not in ("step", "grad", "act") for k in want):
            raise ValueError(f"latent_saliency: want={want} -- known: 'step', 'grad', 'act'")
        if presence_col is not None and not 0 <= _as_int(who, presence_col, "presence_col") < d:
            raise ValueError(f"latent_saliency: presence_col={presence_col} outside [0, d={d})")
        seed_index, seed_full = -1, None
        if isinstance(target, str):
            if target != "argmax":
                raise ValueError(f"latent_saliency: target={target!r} -- 'argmax', an int or a tensor [E, W, nA, N, Z]")
        elif _is_int(target):
            seed_index = int(target)
            if not 0 <= seed_index < Z:
                raise ValueError(f"latent_saliency: target={seed_index} outside [0, Z={Z})")
        elif isinstance(target, np.ndarray) or torch.is_tensor(target):
            if tuple(target.shape) != (E, W, nA, N, Z) or not (torch.as_tensor(target).dtype.is_floating_point):
                raise ValueError(f"latent_saliency: a target tensor must be float [E, W, nA, N, Z] = {(E, W, nA, N, Z)}, got {tuple(target.shape)}")
            seed_full = _as_dev(target, dev)
        else:
            raise ValueError(f"latent_saliency: target={target!r} -- 'argmax', an int or a tensor [E, W, nA, N, Z]")
        if not (isinstance(max_workspace_mb, (int, float)) and max_workspace_mb > 0):
            raise ValueError(f"latent_saliency: max_workspace_mb={max_workspace_mb!r} must be positive")

        hist = _net_major(_as_dev(history, dev), d)
        names = ["step_l1", "carry_l2", "latent"]
        names += ["step_gxi", "feature_l1"] if "step" in want else []
        names += ["grad"] if "grad" in want else []
        names += ["active"] if "act" in want else []
        names += ["target_index"] if seed_full is None and seed_index < 0 else []
        tail = dict(grad=(R, d), step_l1=(R,), step_gxi=(R,), feature_l1=(d,), carry_l2=(), latent=(Z,), target_index=(), active=(K + 1, Lw))
        # chunks: envs first; where ONE env with all windows does not fit, groups of windows as well.  Counted against the limit: the
        # kernel's scratch (he_j of windows 0 .. max(windows), one index per slot) and the chunk's own output buffers.
        out_w = nA * N * sum(int(np.prod(tail[k])) for k in names)                  # output floats per env and window
        he_env = ops.enc_saliency_scratch_floats(nA, N, win[-1:]) - nA * N           # scratch floats per env that all windows share
        Ec, groups = _chunks(who, E, W, he_env, nA * N + out_w, max_workspace_mb, "window")
        full = {k: torch.empty((nA, E, N, W) + tail[k], dtype=torch.int32 if k in ("target_index", "active") else torch.float32, device=dev)
                for k in names}
        for e0 in range(0, E, Ec):
            e1 = min(E, e0 + Ec)
            for w0, w1 in groups:
                seed = None
                if seed_full is not None:
                    seed = seed_full[e0:e1, w0:w1].permute(2, 0, 3, 1, 4).reshape(nA, (e1 - e0) * N, w1 - w0, Z).contiguous()
                out = ops.enc_saliency(self.enc_arena, hist[:, e0:e1], win[w0:w1], K, Lw, Z, self.soft_update_coef, seed=seed,
                                       seed_index=seed_index, want=names)
                for k in names:
                    full[k][:, e0:e1, :, w0:w1] = out[k].reshape((nA, e1 - e0, N, w1 - w0) + tail[k])
        jw = torch.tensor(win, device=dev)
        r = torch.arange(R, device=dev)
        Kj = torch.clamp(jw, max=K)
        step_valid = (r[None, :] <= jw[:, None]) & (r[None, :] <= (Kj + Lw - 1)[:, None])         # [W, R]
        counted = step_valid[None, None, None].expand(nA, E, N, W, R)
        if presence_col is not None:
            counted = counted & (hist[..., presence_col].index_select(2, jw).permute(0, 1, 3, 2) != 0)[..., None]
        cnt = counted.sum(dim=(1, 2, 3)).double()                                                 # [nA, R]
        num = (full["step_l1"].double() * counted).sum(dim=(1, 2, 3))
        lag_l1 = torch.where(cnt > 0, num / cnt.clamp(min=1.0), torch.zeros_like(num))
        res = {k: full[k].permute(*((1, 3, 0, 2) + tuple(range(4, full[k].dim())))) for k in names}
        if "step" not in want:
            del res["step_l1"]
        if "active" in res:
            res["active"] = res["active"].to(torch.int64) & 0xFFFFFFFF
        if "target_index" in res:
            res["target_index"] = res["target_index"].to(torch.int64)
        res["step_valid"], res["lag_l1"] = step_valid, lag_l1
        return _to_numpy(res) if as_np else res

    def latent_knockout(self, history, starts, duration=1, horizon=None, columns=None, baseline=None, want=("shift",), presence_col=0,
                        max_workspace_mb=256):
        """How far a vehicle's intent moves, whether its argmax intent changes, and for how many windows the encoder remembers, when
        the encoder does not see some steps (or some columns) of the RAW history: the finite counterpart of ``latent_saliency``, on
        the chain ``latent_trace`` walks (csrc/enc_knockout.hip; no decoder is run).  history [E, T, nA, N, d] as for ``latent_trace``
        (numpy in -> numpy out, device tensor in -> device tensors out); L = max_history_len, J = T - 1 - L.
          starts    an int or a sorted sequence of distinct ints in [0, J); Q = their number, one job per entry
          duration  D >= 1: job q with start s replaces, for every vehicle chain at once (a vehicle's rows feed only its own latent),
                    the selected columns of steps s .. s+D-1; steps that no reported window reads are harmless
          columns   None = all d, or a sequence of distinct ints in [0, d)
          baseline  None = zeros (the observation wrapper's encoding of an unseen vehicle), a float row [d] or [nA, d], or "hold" =
                    the vehicle's own row of step s-1 (zeros when s = 0)
          horizon   H >= 1, None = J - min(starts): job q reports windows s_q + h, h < H.  Entries with s_q + h >= J do not exist:
                    they are exactly 0 / False and marked in window_valid
          want      any of "shift", "latent_ko", "hidden_ko" (only adds)
        The knocked chain starts from the base chain's he_{s-1}, lat_{s-1}.  Windows s .. s+D+L-2 read a replaced row; later ones
        differ only through the carried state and the averaged latent.  Returns a dict, pair axes [E, H, nA, Q, N]:
          latent        [E, Jn, nA, N, Z]  the base chain, Jn = min(J, max(starts) + H): bit for bit a prefix of ``latent_trace``'s
          intent_base   [E, Jn, nA, N] int64  its argmax (lowest index on ties)
          latent_shift, state_shift   || lat_ko - lat ||_2 and || he_ko - he ||_2 at the same window
          intent, flip  int64 argmax of the knocked latent; intent != intent_base at the same window
          latent_ko [.., Z], hidden_ko [.., 32]   the knocked chain itself ("latent_ko" / "hidden_ko"): latent_ko of job q is what
                        ``latent_trace`` returns at windows s_q .. on an explicitly modified copy
          starts [Q] int64, window = (D, H), direct_windows = min(H, D + L - 1), window_valid [Q, H] bool, columns [.] int64
          echo_shift, echo_flip_rate [nA, Q, H] float64 ("shift"): the mean of latent_shift / flip over the (env, vehicle) pairs of
                        valid windows whose vehicle is present (history[e, t, a, n, presence_col] != 0) in at least one knocked step
                        t < T -- every pair with presence_col=None; 0 where nothing counts
        Envs (and, where one env does not fit, jobs) are processed in chunks so that workspace plus the chunk's outputs stay under
        ``max_workspace_mb``; chunked and unchunked calls give the same bits.  Deterministic; draws from no generator; no parameter,
        gradient, optimiser or carried state is touched; a data-parallel ``dp`` attachment is not consulted."""
        self.join_decoder()
        who = "latent_knockout"
        as_np, E, T, nA, N, d, J = _history_dims(who, "iplan_enc_knockout", self, history)
        Lw, Z, dev = self.max_history_len, self.latent_dim, self.device
        st = _int_list(who, starts, "starts", "an entry of starts")
        _sorted_inside(who, st, "starts", J)
        Q = len(st)
        D = _as_int(who, duration, "duration")
        if D < 1:
            raise ValueError(f"latent_knockout: duration={D} must be at least 1")
        H = J - st[0] if horizon is None else _as_int(who, horizon, "horizon")
        if H < 1:
            raise ValueError(f"latent_knockout: horizon={H} must be at least 1")
        if columns is None:
            cols = list(range(d))
        else:
            if isinstance(columns, (int, np.integer)):
                raise ValueError(f"latent_knockout: columns must be None or a sequence of ints, got {columns!r}")
            cols = _int_list(who, columns, "columns", "an entry of columns")
            if not cols or any(c < 0 or c >= d for c in cols) or len(set(cols)) != len(cols):
                raise ValueError(f"latent_knockout: columns must be distinct and inside [0, d={d}), got {cols}")
        want = (want,) if isinstance(want, str) else tuple(want)
        if any(k not in ("shift", "latent_ko", "hidden_ko") for k in want):
            raise ValueError(f"latent_knockout: want={want} -- known: 'shift', 'latent_ko', 'hidden_ko'")
        if presence_col is not None and not 0 <= _as_int(who, presence_col, "presence_col") < d:
            raise ValueError(f"latent_knockout: presence_col={presence_col} outside [0, d={d})")
        hold, base_row = False, None
        if isinstance(baseline, str):
            if baseline != "hold":
                raise ValueError(f"latent_knockout: baseline={baseline!r} -- None, 'hold', or a float row [d] or [nA, d]")
            hold = True
        elif baseline is not None:
            try:
                b = torch.as_tensor(baseline)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"latent_knockout: baseline={baseline!r} -- None, 'hold', or a float row [d] or [nA, d]") from None
            if not b.dtype.is_floating_point or tuple(b.shape) not in ((d,), (nA, d)):
                raise ValueError(f"latent_knockout: a baseline row must be float [d] or [nA, d] = {(nA, d)}, got {b.dtype} {tuple(b.shape)}")
            base_row = b.to(device=dev, dtype=torch.float32).expand(nA, d).contiguous()
        if isinstance(max_workspace_mb, (bool, np.bool_)) or not (isinstance(max_workspace_mb, (int, float)) and max_workspace_mb > 0):
            raise ValueError(f"latent_knockout: max_workspace_mb={max_workspace_mb!r} must be positive")

        hist = _net_major(_as_dev(history, dev), d)
        Jn = ops.enc_knockout_windows(J, st, H)
        names = ["latent", "intent_base", "intent", "latent_shift_sq", "state_shift_sq"]
        names += [k for k in ("latent_ko", "hidden_ko") if k in want]
        tail = dict(intent=(), latent_shift_sq=(), state_shift_sq=(), latent_ko=(Z,), hidden_ko=(32,))
        # chunks: envs first; where ONE env with all jobs does not fit, groups of jobs as well (each group walks the base chain as far
        # as it needs).  Counted against the limit: the kernel's workspace (he_j of windows 0 .. Jn-1), the base chain's outputs and
        # the chunk's per-job outputs.
        slot = nA * N * H * sum(int(np.prod(tail[k])) for k in names[2:])           # output floats per env and job
        base_env = nA * N * Jn * (32 + Z + 1)                                       # workspace and base outputs per env
        Ec, groups = _chunks(who, E, Q, base_env, slot, max_workspace_mb, "job")
        f32, i32 = torch.float32, torch.int32
        full = {k: torch.zeros((nA, E, N, Q, H) + tail[k], dtype=i32 if k == "intent" else f32, device=dev) for k in names[2:]}
        full["latent"] = torch.empty(nA, E, N, Jn, Z, dtype=f32, device=dev)
        full["intent_base"] = torch.empty(nA, E, N, Jn, dtype=i32, device=dev)
        for e0 in range(0, E, Ec):
            e1 = min(E, e0 + Ec)
            for q0, q1 in groups:
                last = q1 == Q                                                       # the group that walks all Jn base windows
                out = ops.enc_knockout(self.enc_arena, hist[:, e0:e1], st[q0:q1], D, H, Lw, Z, self.soft_update_coef, columns=cols,
                                       baseline=base_row, hold=hold, want=names if last else names[2:])
                for k in names[2:]:
                    full[k][:, e0:e1, :, q0:q1] = out[k].reshape((nA, e1 - e0, N, q1 - q0, H) + tail[k])
                if last:
                    full["latent"][:, e0:e1] = out["latent"].reshape(nA, e1 - e0, N, Jn, Z)
                    full["intent_base"][:, e0:e1] = out["intent_base"].reshape(nA, e1 - e0, N, Jn)
        sq = torch.tensor(st, device=dev)
        win = sq[:, None] + torch.arange(H, device=dev)[None, :]                                   # [Q, H]: the window of every slot
        window_valid = win < J
        pair = lambda t: t.permute(*((1, 4, 0, 3, 2) + tuple(range(5, t.dim()))))                  # [nA, E, N, Q, H, ..] -> [E, H, nA, Q, N, ..]
        intent_base = full["intent_base"].to(torch.int64)
        intent = full["intent"].to(torch.int64)
        flip = (intent != intent_base[..., win.clamp(max=Jn - 1)]) & window_valid
        res = {"latent": full["latent"].permute(1, 3, 0, 2, 4), "intent_base": intent_base.permute(1, 3, 0, 2),
               "latent_shift": pair(torch.sqrt(full["latent_shift_sq"])), "state_shift": pair(torch.sqrt(full["state_shift_sq"])),
               "intent": pair(intent), "flip": pair(flip)}
        for k in ("latent_ko", "hidden_ko"):
            if k in want:
                res[k] = pair(full[k])
        res["starts"], res["window_valid"], res["columns"] = sq, window_valid, torch.tensor(cols, device=dev)
        if "shift" in want:
            # the pairs that count: the vehicle is present in at least one knocked step t < T (a difference of running counts)
            if presence_col is None:
                counted = torch.ones(nA, E, Q, N, dtype=torch.bool, device=dev)
            else:
                seen = (hist[..., presence_col] != 0).to(torch.int64).cumsum(dim=2)                # [nA, E, T, N]
                seen = torch.cat([torch.zeros_like(seen[:, :, :1]), seen], dim=2)
                counted = (seen[:, :, (sq + D).clamp(max=T)] - seen[:, :, sq]) > 0                 # [nA, E, Q, N]
            counted = counted[:, :, :, None, :] & window_valid[None, None, :, :, None]             # [nA, E, Q, H, N]
            shift64 = res["latent_shift"].permute(2, 0, 3, 1, 4).double()                          # [nA, E, Q, H, N]
            flip64 = res["flip"].permute(2, 0, 3, 1, 4).double()
            # float64 sums in a fixed order: environments ascending, then vehicles ascending
            num = torch.zeros(2, nA, Q, H, N, dtype=torch.float64, device=dev)
            cnt = torch.zeros(nA, Q, H, N, dtype=torch.float64, device=dev)
            for e in range(E):
                w = counted[:, e].double()
                num = num + torch.stack([shift64[:, e] * w, flip64[:, e] * w])
                cnt = cnt + w
            tot, ctot = num[..., 0], cnt[..., 0]
            for i in range(1, N):
                tot, ctot = tot + num[..., i], ctot + cnt[..., i]
            mean = torch.where(ctot > 0, tot / ctot.clamp(min=1.0), torch.zeros_like(tot))
            res["echo_shift"], res["echo_flip_rate"] = mean[0], mean[1]
        meta = {"window": (D, H), "direct_windows": min(H, D + Lw - 1)}
        if as_np:
            res = _to_numpy(res)
        res.update(meta)
        return res

    # ---------------------------------------------------------------------------- checkpoints
    def save_models(self, path):
        self.join_decoder()
        for i in range(self.n_agents):
            torch.save(self.behavior_encoder[i].state_dict(), f"{path}/behavior_encoder_{i}.th")
            torch.save(self.behavior_decoder[i].state_dict(), f"{path}/behavior_decoder_{i}.th")
            torch.save(self.behavior_optimizer[i].state_dict(), f"{path}/behavior_optimizer_{i}_opt.th")

    def load_models(self, paths, load_optimisers=False):
        self.join_decoder()
        if len(paths) == 1:
            paths = [copy.copy(paths[0]) for _ in range(self.n_agents)]
        for i in range(self.n_agents):
            self.behavior_encoder[i].load_state_dict(
                torch.load(f"{paths[i]}/behavior_encoder_{i}.th", map_location="cpu"))
            self.behavior_decoder[i].load_state_dict(
                torch.load(f"{paths[i]}/behavior_decoder_{i}.th", map_location="cpu"))
            if load_optimisers:
                self.behavior_optimizer[i].load_state_dict(
                    torch.load(f"{paths[i]}/behavior_optimizer_{i}_opt.th", map_location="cpu"))
