"""Host-side launch wrappers: torch tensors in, C-ABI structs out.

Each function only (a) allocates outputs with torch, (b) fills the argument struct with raw device
pointers / strides, (c) calls the entry point on torch's current stream.  No arithmetic happens
here.  ``lib`` defaults to the gfx950 build; the CPU test-suite passes the host-emulated build of
the same kernel sources instead.
"""
import contextlib
import ctypes as C

import os

import torch

from . import _lib as L


def _lib(lib):
    return lib if lib is not None else L.get_lib()


def _nb_strides(t, inner):
    """t is logically [n_nets, B, <inner dims contiguous>]; returns (s_net, s_b) in elements."""
    assert t.dtype == torch.float32, t.dtype
    expect = 1
    for d in range(t.dim() - 1, 1, -1):
        assert t.stride(d) == expect or t.shape[d] == 1, (t.shape, t.stride())
        expect *= t.shape[d]
    assert expect == inner, (expect, inner)
    return t.stride(0), t.stride(1)


def _gat_flops(n_nets, B, N, D, A, H=32):
    """algorithmic FLOPs of one GAT forward: V (2DH + 24H^2 + 6HA + 12A^2) + P (12H^2 + 8H + 4A) per net"""
    V, P = B * N, B * N * (N - 1)
    return float(n_nets * (V * (2 * D * H + 24 * H * H + 6 * H * A + 12 * A * A) + P * (12 * H * H + 8 * H + 4 * A)))


def gat_forward(arena, src0, src1, h_prev, noise, tau=0.01, save=False, out=None, phase_clocks=None, lib=None, fuse_enc=None, fuse_ac=None):
    """GAT_Net.forward for all nets.  src0 [n_nets,B,N,d0], src1 [n_nets,B,N,d1] or None,
    h_prev [n_nets,B,N,A] (first two dims may be arbitrarily strided views), noise
    [n_nets,B,N,N-1,2] contiguous.  Returns (out [n_nets,B,N,A], saved dict or None).
    ``fuse_enc``: what ``enc_forward(..., launch=False)`` returned -- the encoder's latent update of the same rollout step rides
    in this launch (iplan_gat_enc_fwd: the GAT scenes' workgroups first, the encoder's behind them).
    ``fuse_ac`` (with ``fuse_enc``): what ``ac_forward(..., launch=False)`` returned for the NEXT step's action selection -- it
    reads what this launch writes and runs as its last workgroups (iplan_gat_enc_ac_fwd)."""
    lib = _lib(lib)
    n_nets, B, N, d0 = src0.shape
    d1 = 0 if src1 is None else src1.shape[-1]
    A = h_prev.shape[-1]
    dev = src0.device
    a = L.GatFwdArgs()
    a.n_nets, a.B, a.N, a.d0, a.d1 = n_nets, B, N, d0, d1
    a.src0 = src0.data_ptr()
    a.src0_s_net, a.src0_s_b = _nb_strides(src0, N * d0)
    if src1 is not None:
        a.src1 = src1.data_ptr()
        a.src1_s_net, a.src1_s_b = _nb_strides(src1, N * d1)
    a.h_prev = h_prev.data_ptr()
    a.h_s_net, a.h_s_b = _nb_strides(h_prev, N * A)
    if out is None:
        out = torch.empty(n_nets, B, N, A, dtype=torch.float32, device=dev)
    a.out = out.data_ptr()
    a.out_s_net, a.out_s_b = _nb_strides(out, N * A)
    assert noise.is_contiguous() and noise.shape == (n_nets, B, N, N - 1, 2), noise.shape
    a.noise = noise.data_ptr()
    a.params = arena.data.data_ptr()
    a.params_s_net = arena.net_stride
    for i, k in enumerate(L.GAT_PARAM_ORDER):
        a.off[i] = arena.off(k)
    a.tau = tau
    if phase_clocks is not None:
        assert phase_clocks.dtype == torch.int64 and phase_clocks.numel() >= n_nets * B * 5
        a.phase_clocks = phase_clocks.data_ptr()
    saved = None
    if save:
        H = A
        saved = dict(
            h_enc=torch.empty(n_nets, B * N, H, device=dev),
            gru=torch.empty(n_nets, 2, B, (N + 15) // 16, N - 1, L.GAT_REC_GROUPS, 16, 16, device=dev),   # tile-major 1 KiB blocks: h r z n (csrc/gat.hip, gat_bwd.hip: REC = 8 * 256 floats per (tile, step))
            qkv=torch.empty(n_nets, B * N, 3 * A, device=dev),
            soft=torch.empty(n_nets, B * N, N - 1, device=dev),
            hard=torch.empty(n_nets, B * N, N - 1, device=dev),
            x=torch.empty(n_nets, B * N, A, device=dev),
            cell=torch.empty(n_nets, B * N, 4 * A, device=dev),
        )
        for k, v in saved.items():
            setattr(a.saved, k, v.data_ptr())
    if fuse_enc is not None and fuse_ac is not None:
        sync = _fused_sync(dev)
        if TIMERS is not None and phase_clocks is None and TIMERS.sample("gat_scenes_clocks", 32):
            # bench.py's roofline: in-kernel stamps of the scenes (entry / end of every scene workgroup, wall_clock64 = 100 MHz) of
            # every 32nd fused launch -- the launch's own duration also holds the next step's action selection behind them
            clocks = torch.zeros(n_nets * B * 5, dtype=torch.int64, device=dev)
            a.phase_clocks = clocks.data_ptr()
            TIMERS.clocks.setdefault("gat_scenes_clocks", []).append(clocks)

        def fused3():
            rc = lib.c.iplan_gat_enc_ac_fwd(C.byref(a), C.byref(fuse_enc["args"]), C.byref(fuse_ac["_args"]), C.c_void_p(sync.data_ptr()),
                                            C.c_void_p(L.current_stream(dev) or 0))
            if rc != 0:
                raise L.IplanError(f"iplan_gat_enc_ac_fwd failed ({rc}): {lib.c.iplan_last_error().decode()}")
        _launch("gat_enc_ac_fwd_kernel", fused3)
    elif fuse_enc is not None:
        assert fuse_ac is None
        def fused():
            rc = lib.c.iplan_gat_enc_fwd(C.byref(a), C.byref(fuse_enc["args"]), C.c_void_p(L.current_stream(dev) or 0))
            if rc != 0:
                raise L.IplanError(f"iplan_gat_enc_fwd failed ({rc}): {lib.c.iplan_last_error().decode()}")
        _launch("gat_fwd_kernel", fused, work=_gat_flops(n_nets, B, N, d0 + d1, A))
    else:
        _launch("gat_fwd_kernel", lambda: lib.call("iplan_gat_fwd", a, L.current_stream(dev)), work=_gat_flops(n_nets, B, N, d0 + d1, A))
    if saved is not None:
        saved["_args"] = a
        saved["_keep"] = (src0, src1, h_prev, noise, out)
    return out, saved


def _room(t):
    """elements from t's first element to the end of its storage"""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _nbs_strides(t, inner, what):
    """t is logically [n_nets, B, S, <inner dims contiguous>] with non-negative strides; returns (s_net, s_b, s_step) in elements
    after checking on the host that the last element the kernel can touch lies inside t's storage."""
    assert t.dtype == torch.float32, (what, t.dtype)
    expect = 1
    for d in range(t.dim() - 1, 2, -1):
        assert t.stride(d) == expect or t.shape[d] == 1, (what, t.shape, t.stride())
        expect *= t.shape[d]
    assert expect == inner, (what, expect, inner)
    s = t.stride()[:3]
    assert all(x >= 0 for x in s), (what, s)
    reach = sum((t.shape[d] - 1) * s[d] for d in range(3)) + inner
    assert reach <= _room(t), (what, "reaches outside its storage", t.shape, s, _room(t))
    return s


def _dest_nbs(out, res, k, lead, inner, dev):
    """``out[k]`` if the caller gave one, else a fresh tensor: float32 [*lead, *inner] whose dims before ``inner`` may be strided (lead =
    (n_nets, B) or (n_nets, B, S)); entered into ``res``, checked to lie inside its storage -> (tensor, s_net, s_b, s_step)"""
    t = None if out is None else out.get(k)
    if t is None:
        t = torch.empty(*lead, *inner, dtype=torch.float32, device=dev)
    assert t.shape == tuple(lead) + tuple(inner) and t.device == dev, (k, t.shape)
    n_in = 1
    for x in inner:
        n_in *= x
    res[k] = t
    return (t,) + tuple(_nbs_strides(t if len(lead) == 3 else t.unsqueeze(2), n_in, k))


GAT_TRACE_OUTPUTS = ("latent", "soft", "hard", "attn", "stats")


def gat_trace(arena, src0, src1=None, hidden0=None, noise=None, tau=0.01, want=("latent",), weight=None, presence_col=-1, out=None,
              lib=None):
    """GAT_Net.forward walked over S consecutive steps in ONE launch (iplan_gat_trace), forward only: h_s = GAT([src0_s ||
    src1_s], h_{s-1}), h_{-1} = hidden0 (None: zeros).  src0 [n_nets,B,S,N,d0], src1 [n_nets,B,S,N,d1] or None: views whose first
    three dims may be strided arbitrarily (episode fields, read in place).  hidden0 [n_nets,B,N,A] (first two dims strided),
    noise [n_nets,B,S,N,N-1,2] contiguous or None (no gumbel term), weight [n_nets,B,S] contiguous or None, ``presence_col``: the
    column of src0 that marks a present entity (< 0: all).  ``want``: which of latent [n_nets,B,S,N,A], soft / hard / attn
    [n_nets,B,S,N,N] (entity-indexed, diagonal 0), stats [n_nets,B,S,6] to produce; ``out``: optional dict of destination views for
    some of them (the same layouts, first three dims strided).  Everything the kernel will touch is bounds-checked here, on
    the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res = gat_trace_args(arena, src0, src1, hidden0, noise, tau, want, weight, presence_col, out)
    n_nets, B, S, N, d0 = src0.shape
    d1 = 0 if src1 is None else src1.shape[-1]
    _launch("gat_trace_kernel", lambda: lib.call("iplan_gat_trace", a, L.current_stream(src0.device)), work=S * _gat_flops(n_nets, B, N, d0 + d1, 32))
    return res


def gat_trace_args(arena, src0, src1=None, hidden0=None, noise=None, tau=0.01, want=("latent",), weight=None, presence_col=-1, out=None):
    """The descriptor of a ``gat_trace`` launch and its output tensors, checked but not launched: (IplanGatTraceArgs, dict).  The
    caller keeps the operands alive until the launch has been queued."""
    n_nets, B, S, N, d0 = src0.shape
    d1 = 0 if src1 is None else src1.shape[-1]
    A = 32
    dev = src0.device
    want = tuple(want)
    assert want and all(k in GAT_TRACE_OUTPUTS for k in want), want
    a = L.GatTraceArgs()
    a.n_nets, a.B, a.N, a.d0, a.d1, a.S = n_nets, B, N, d0, d1, S
    a.src0 = src0.data_ptr()
    a.src0_s_net, a.src0_s_b, a.src0_s_step = _nbs_strides(src0, N * d0, "src0")
    if src1 is not None:
        assert src1.shape[:4] == (n_nets, B, S, N) and src1.device == dev, src1.shape
        a.src1 = src1.data_ptr()
        a.src1_s_net, a.src1_s_b, a.src1_s_step = _nbs_strides(src1, N * d1, "src1")
    if hidden0 is not None:
        assert hidden0.shape == (n_nets, B, N, A) and hidden0.device == dev, hidden0.shape
        a.hidden0 = hidden0.data_ptr()
        a.h_s_net, a.h_s_b, _ = _nbs_strides(hidden0.unsqueeze(2), N * A, "hidden0")
    if noise is not None:
        assert noise.is_contiguous() and noise.shape == (n_nets, B, S, N, N - 1, 2) and noise.dtype == torch.float32 and noise.device == dev, noise.shape
        a.noise = noise.data_ptr()
    if weight is not None:
        assert weight.is_contiguous() and weight.shape == (n_nets, B, S) and weight.dtype == torch.float32 and weight.device == dev, weight.shape
        a.weight = weight.data_ptr()
    assert presence_col < d0
    a.presence_col = max(int(presence_col), -1)
    a.params = arena.data.data_ptr()
    a.params_s_net = arena.net_stride
    for i, k in enumerate(L.GAT_PARAM_ORDER):
        a.off[i] = arena.off(k)
    a.tau = tau
    res = {}
    for k in want:
        inner = {"latent": (N, A), "stats": (L.GAT_TRACE_NSTAT,)}.get(k, (N, N))
        t, *s = _dest_nbs(out, res, k, (n_nets, B, S), inner, dev)
        setattr(a, k, t.data_ptr())
        if k == "stats":
            assert t.is_contiguous()
        else:
            pre = "lat" if k == "latent" else k
            for name, v in zip(("net", "b", "step"), s):
                setattr(a, f"{pre}_s_{name}", v)
    return a, res


GAT_KNOCKOUT_OUTPUTS = ("latent_ko", "attn_ko", "shift_sq")


def gat_knockout(arena, src0, src1, hidden, jobs, base=None, noise=None, tau=0.01, knock=(True, True), baseline=(None, None),
                 want=("shift_sq",), out=None, lib=None):
    """Every scene run once per job with one entity's input row replaced (iplan_gat_knockout), forward only.  src0 [n_nets,B,N,d0],
    src1 [n_nets,B,N,d1] or None, hidden [n_nets,B,N,A] or None (zeros): views whose first two dims may be strided arbitrarily, read in
    place.  ``jobs``: J entity indices in [0, N), or -1 for "nothing knocked" (duplicates allowed), shared by all scenes.  ``knock``:
    which of (src0, src1) is replaced in the knocked row, by ``baseline`` = (row [d0] or None, row [d1] or None), None = zeros.
    ``noise`` [n_nets,B,N,N-1,2] contiguous or None (no gumbel term): the same samples for every job of a scene.  ``want``: which of
    latent_ko [n_nets,B,J,N,A], attn_ko [n_nets,B,J,N,N] (entity-indexed soft * hard, diagonal 0), shift_sq [n_nets,B,J,N] (sum_c
    (latent_ko - base)^2; needs ``base`` [n_nets,B,N,A], first two dims strided, produced by an earlier launch) to produce; ``out``:
    optional dict of destination views for some of them (the same layouts, first three dims strided).  Everything the kernel will
    touch is bounds-checked here, on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, keep = gat_knockout_args(arena, src0, src1, hidden, jobs, base, noise, tau, knock, baseline, want, out)
    n_nets, B, N, d0 = src0.shape
    _launch("gat_knockout_kernel", lambda: lib.call("iplan_gat_knockout", a, L.current_stream(src0.device)),
            work=a.J * _gat_flops(n_nets, B, N, d0 + a.d1, 32))
    res["_keep"] = keep
    return res


def gat_knockout_args(arena, src0, src1, hidden, jobs, base=None, noise=None, tau=0.01, knock=(True, True), baseline=(None, None),
                      want=("shift_sq",), out=None):
    """The descriptor of a ``gat_knockout`` launch, its output tensors and what must stay alive until the launch has been queued,
    checked but not launched: (IplanGatKnockoutArgs, dict, list)."""
    n_nets, B, N, d0 = src0.shape
    d1 = 0 if src1 is None else src1.shape[-1]
    A = 32
    dev = src0.device
    want = tuple(want)
    assert want and all(k in GAT_KNOCKOUT_OUTPUTS for k in want), want
    k0, k1 = bool(knock[0]), bool(knock[1])
    assert not (k1 and d1 == 0), "source 1 is to be knocked, but there is none"
    a = L.GatKnockoutArgs()
    a.n_nets, a.B, a.N, a.d0, a.d1 = n_nets, B, N, d0, d1
    j_host, j_dev = _job_list(a, jobs, N, dev)
    J = a.J
    a.src0 = src0.data_ptr()
    a.src0_s_net, a.src0_s_b, _ = _nbs_strides(src0.unsqueeze(2), N * d0, "src0")
    if src1 is not None:
        assert src1.shape[:3] == (n_nets, B, N) and src1.device == dev, src1.shape
        a.src1 = src1.data_ptr()
        a.src1_s_net, a.src1_s_b, _ = _nbs_strides(src1.unsqueeze(2), N * d1, "src1")
    if hidden is not None:
        assert hidden.shape == (n_nets, B, N, A) and hidden.device == dev, hidden.shape
        a.hidden = hidden.data_ptr()
        a.h_s_net, a.h_s_b, _ = _nbs_strides(hidden.unsqueeze(2), N * A, "hidden")
    if noise is not None:
        assert noise.is_contiguous() and noise.shape == (n_nets, B, N, N - 1, 2) and noise.dtype == torch.float32 and noise.device == dev, noise.shape
        a.noise = noise.data_ptr()
    if base is not None:
        assert base.shape == (n_nets, B, N, A) and base.device == dev, base.shape
        a.base = base.data_ptr()
        a.base_s_net, a.base_s_b, _ = _nbs_strides(base.unsqueeze(2), N * A, "base")
    assert "shift_sq" not in want or base is not None, "shift_sq needs base, the latent with nothing knocked"
    a.knock0, a.knock1 = int(k0), int(k1)
    keep = [src0, src1, hidden, noise, base, j_host, j_dev]
    for which, (row, d) in enumerate(zip(baseline, (d0, d1))):
        if row is not None:
            assert row.shape == (d,) and row.dtype == torch.float32 and row.is_contiguous() and row.device == dev, (which, row.shape)
            setattr(a, f"baseline{which}", row.data_ptr())
            keep.append(row)
    a.params = arena.data.data_ptr()
    a.params_s_net = arena.net_stride
    for i, k in enumerate(L.GAT_PARAM_ORDER):
        a.off[i] = arena.off(k)
    a.tau = tau
    res = {}
    pre = {"latent_ko": "lat", "attn_ko": "attn", "shift_sq": "shift"}
    for k in want:
        inner = {"latent_ko": (N, A), "attn_ko": (N, N), "shift_sq": (N,)}[k]
        t, *s = _dest_nbs(out, res, k, (n_nets, B, J), inner, dev)
        setattr(a, k, t.data_ptr())
        for name, v in zip(("net", "b", "job"), s):
            setattr(a, f"{pre[k]}_s_{name}", v)
    return a, res, keep


def _dest_nbjs(out, res, k, lead, inner, dev):
    """``out[k]`` if the caller gave one, else a fresh tensor: float32 [n_nets, B, J, H, *inner] whose four leading dims may be strided
    (non-negative); entered into ``res``, checked to lie inside its storage -> (tensor, s_net, s_b, s_job, s_step)"""
    t = None if out is None else out.get(k)
    if t is None:
        t = torch.empty(*lead, *inner, dtype=torch.float32, device=dev)
    assert t.shape == tuple(lead) + tuple(inner) and t.device == dev and t.dtype == torch.float32, (k, t.shape, t.dtype)
    expect = 1
    for d in range(t.dim() - 1, 3, -1):
        assert t.stride(d) == expect or t.shape[d] == 1, (k, t.shape, t.stride())
        expect *= t.shape[d]
    s = t.stride()[:4]
    assert all(x >= 0 for x in s), (k, s)
    reach = sum((t.shape[d] - 1) * s[d] for d in range(4)) + expect
    assert reach <= _room(t), (k, "reaches outside its storage", t.shape, s, _room(t))
    res[k] = t
    return (t,) + tuple(s)


def gat_knockout_trace(arena, src0, src1, hidden0, jobs, start=0, duration=1, horizon=None, base=None, noise=None, tau=0.01,
                       knock=(True, True), baseline=(None, None), want=("shift_sq",), out=None, lib=None):
    """``gat_trace``'s walk run once per job with one entity's input row replaced in the first ``duration`` steps of the window
    (iplan_gat_knockout_trace), forward only.  src0 [n_nets,B,S,N,d0], src1 [n_nets,B,S,N,d1] or None: the episode fields, views whose
    first three dims may be strided arbitrarily, read in place; the window is steps start .. start + H - 1 (``horizon`` None: H = S -
    start).  hidden0 [n_nets,B,N,A] or None (zeros): the state step ``start`` starts from (first two dims strided).  ``jobs``,
    ``knock``, ``baseline``: as in ``gat_knockout``.  ``noise`` [n_nets,B,H,N,N-1,2] contiguous or None (no gumbel term): the window's
    samples, the same for every job.  ``want``: which of latent_ko [n_nets,B,J,H,N,A], attn_ko [n_nets,B,J,H,N,N] (entity-indexed soft
    * hard, diagonal 0), shift_sq [n_nets,B,J,H,N] (sum_c (latent_ko - base)^2; needs ``base`` [n_nets,B,H,N,A], first three dims
    strided: ``gat_trace``'s latent over the same window, produced by an earlier launch) to produce; ``out``: optional dict of
    destination views for some of them (the same layouts, first four dims strided).  Everything the kernel will touch is
    bounds-checked here, on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, keep = gat_knockout_trace_args(arena, src0, src1, hidden0, jobs, start, duration, horizon, base, noise, tau, knock, baseline, want, out)
    n_nets, B, _, N, d0 = src0.shape
    _launch("gat_knockout_trace_kernel", lambda: lib.call("iplan_gat_knockout_trace", a, L.current_stream(src0.device)),
            work=a.J * a.H * _gat_flops(n_nets, B, N, d0 + a.d1, 32))
    res["_keep"] = keep
    return res


def gat_knockout_trace_args(arena, src0, src1, hidden0, jobs, start=0, duration=1, horizon=None, base=None, noise=None, tau=0.01,
                            knock=(True, True), baseline=(None, None), want=("shift_sq",), out=None):
    """The descriptor of a ``gat_knockout_trace`` launch, its output tensors and what must stay alive until the launch has been
    queued, checked but not launched: (IplanGatKnockoutTraceArgs, dict, list)."""
    n_nets, B, S, N, d0 = src0.shape
    d1 = 0 if src1 is None else src1.shape[-1]
    A = 32
    dev = src0.device
    want = tuple(want)
    assert want and all(k in GAT_KNOCKOUT_OUTPUTS for k in want), want
    k0, k1 = bool(knock[0]), bool(knock[1])
    assert not (k1 and d1 == 0), "source 1 is to be knocked, but there is none"
    start = int(start)
    H = S - start if horizon is None else int(horizon)
    D = int(duration)
    assert 0 <= start and H >= 1 and start + H <= S and 1 <= D <= H, (start, D, H, S)
    a = L.GatKnockoutTraceArgs()
    a.n_nets, a.B, a.N, a.d0, a.d1, a.H, a.D, a.start = n_nets, B, N, d0, d1, H, D, start
    j_host, j_dev = _job_list(a, jobs, N, dev)
    J = a.J
    a.src0 = src0.data_ptr()
    a.src0_s_net, a.src0_s_b, a.src0_s_step = _nbs_strides(src0, N * d0, "src0")
    if src1 is not None:
        assert src1.shape[:4] == (n_nets, B, S, N) and src1.device == dev, src1.shape
        a.src1 = src1.data_ptr()
        a.src1_s_net, a.src1_s_b, a.src1_s_step = _nbs_strides(src1, N * d1, "src1")
    if hidden0 is not None:
        assert hidden0.shape == (n_nets, B, N, A) and hidden0.device == dev, hidden0.shape
        a.hidden0 = hidden0.data_ptr()
        a.h_s_net, a.h_s_b, _ = _nbs_strides(hidden0.unsqueeze(2), N * A, "hidden0")
    if noise is not None:
        assert noise.is_contiguous() and noise.shape == (n_nets, B, H, N, N - 1, 2) and noise.dtype == torch.float32 and noise.device == dev, noise.shape
        a.noise = noise.data_ptr()
    if base is not None:
        assert base.shape == (n_nets, B, H, N, A) and base.device == dev, base.shape
        a.base = base.data_ptr()
        a.base_s_net, a.base_s_b, a.base_s_step = _nbs_strides(base, N * A, "base")
    assert "shift_sq" not in want or base is not None, "shift_sq needs base, the latents of the window with nothing knocked"
    a.knock0, a.knock1 = int(k0), int(k1)
    keep = [src0, src1, hidden0, noise, base, j_host, j_dev]
    for which, (row, d) in enumerate(zip(baseline, (d0, d1))):
        if row is not None:
            assert row.shape == (d,) and row.dtype == torch.float32 and row.is_contiguous() and row.device == dev, (which, row.shape)
            setattr(a, f"baseline{which}", row.data_ptr())
            keep.append(row)
    a.params = arena.data.data_ptr()
    a.params_s_net = arena.net_stride
    for i, k in enumerate(L.GAT_PARAM_ORDER):
        a.off[i] = arena.off(k)
    a.tau = tau
    res = {}
    pre = {"latent_ko": "lat", "attn_ko": "attn", "shift_sq": "shift"}
    for k in want:
        inner = {"latent_ko": (N, A), "attn_ko": (N, N), "shift_sq": (N,)}[k]
        t, *s = _dest_nbjs(out, res, k, (n_nets, B, J, H), inner, dev)
        setattr(a, k, t.data_ptr())
        for name, v in zip(("net", "b", "job", "step"), s):
            setattr(a, f"{pre[k]}_s_{name}", v)
    return a, res, keep


GAT_SALIENCY_OUTPUTS = ("grad", "pair_gl1", "pair_gxi", "input_grad", "hidden_grad")


def gat_saliency_scratch_floats(n_nets, B, N):
    """floats of scratch an exact-gate ``gat_saliency`` launch needs: [dr dz dn_i] of every pair step of both directions + their sums"""
    return n_nets * B * 2 * N * N * 3 * 32


def gat_saliency(arena, saved, v, gate_through=True, want=("input_grad",), out=None, scratch=None, lib=None):
    """The input backward of a ``gat_forward(..., save=True)`` launch with the egos kept apart (iplan_gat_saliency): for every
    scene and ego i, G[i, j, :] = d <v_i, latent_i> / d [src0 || src1][j].  ``saved``: what that forward returned; v [n_nets,B,N,A]
    (first two dims strided).  ``gate_through=False`` holds the gumbel gate constant (the pair-GRU record is not read).  ``want``:
    which of grad [n_nets,B,N,N,D], pair_gl1 / pair_gxi [n_nets,B,N,N,n_src], input_grad [n_nets,B,N,D], hidden_grad [n_nets,B,N,A]
    to produce; ``out``: optional dict of destination views for some of them (first two dims strided, inside their storage);
    ``scratch``: optional float32 buffer of at least ``gat_saliency_scratch_floats`` floats.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, keep = gat_saliency_args(arena, saved, v, gate_through, want, out, scratch)
    _launch("gat_saliency_kernel", lambda: lib.call("iplan_gat_saliency", a, L.current_stream(v.device)))
    res["_keep"] = keep
    return res


def gat_saliency_args(arena, saved, v, gate_through=True, want=("input_grad",), out=None, scratch=None):
    """The descriptor of a ``gat_saliency`` launch, its output tensors and what must stay alive until the launch has been queued,
    checked but not launched: (IplanGatSaliencyArgs, dict, list)."""
    fa = saved["_args"]
    n_nets, B, N, d0, d1 = fa.n_nets, fa.B, fa.N, fa.d0, fa.d1
    A, D, n_src = 32, d0 + d1, 2 if d1 > 0 else 1
    dev = v.device
    want = tuple(want)
    assert want and all(k in GAT_SALIENCY_OUTPUTS for k in want), want
    assert fa.params == arena.data.data_ptr(), "saved belongs to another arena"
    a = L.GatSaliencyArgs()
    a.fwd = fa
    assert v.shape == (n_nets, B, N, A) and v.dtype == torch.float32, (v.shape, v.dtype)
    a.v = v.data_ptr()
    a.v_s_net, a.v_s_b, _ = _nbs_strides(v.unsqueeze(2), N * A, "v")
    a.gate_through = 1 if gate_through else 0
    keep = [saved, v]
    if gate_through:
        need = gat_saliency_scratch_floats(n_nets, B, N)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.float32, device=dev)
        assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= need and scratch.device == dev, (scratch.numel(), need)
        a.scratch, a.scratch_floats = scratch.data_ptr(), scratch.numel()
        keep.append(scratch)
    res = {}
    inner = {"grad": (N, N, D), "pair_gl1": (N, N, n_src), "pair_gxi": (N, N, n_src), "input_grad": (N, D), "hidden_grad": (N, A)}
    pre = {"grad": "grad", "input_grad": "ig", "hidden_grad": "hg"}
    pair = None
    for k in want:
        t, s_net, s_b, _ = _dest_nbs(out, res, k, (n_nets, B), inner[k], dev)
        setattr(a, k, t.data_ptr())
        if k in pre:
            setattr(a, pre[k] + "_s_net", s_net)
            setattr(a, pre[k] + "_s_b", s_b)
        else:
            assert pair is None or pair == (s_net, s_b), "pair_gl1 and pair_gxi share their strides"
            pair = (s_net, s_b)
            a.pair_s_net, a.pair_s_b = s_net, s_b
    return a, res, keep


GAT_SALIENCY_TRACE_OUTPUTS = ("grad", "pair_gl1", "pair_gxi", "input_grad", "carry", "carry_sq")


def gat_saliency_trace_scratch_floats(n_nets, B, T, N):
    """floats of scratch an exact-gate ``gat_saliency_trace`` launch needs: one ``gat_saliency`` scene's worth per (net, env, target),
    reused by every lag"""
    return n_nets * B * T * 2 * N * N * 3 * 32


def gat_saliency_trace(arena, saved, steps, v, targets, lags=0, gate_through=True, want=("input_grad",), out=None, scratch=None, targets_dev=None,
                       lib=None):
    """``gat_saliency`` chained over the past steps of each ego's own latent (iplan_gat_saliency_trace).  ``saved``: what ONE
    ``gat_forward(..., save=True)`` over rows (env, record step) returned -- B * ``steps`` rows per net, row b * steps + r, its
    ``h_prev`` row the latent of record step r - 1; it is read in place by every target and lag that reaches a row.  ``targets``:
    T record steps in [0, steps); ``lags`` = K >= 0; v [n_nets,B,T,N,A] (first three dims strided): the cotangent of every target.
    For lag k <= min(K, r) the slot holds ``gat_saliency`` on row r - k with the previous lag's ``hidden_grad`` as cotangent (bit for
    bit); the slots of lags k > r are +0.0.  ``want``: which of grad [n_nets,B,T,K+1,N,N,D], pair_gl1 / pair_gxi
    [n_nets,B,T,K+1,N,N,n_src], input_grad [n_nets,B,T,K+1,N,D], carry [n_nets,B,T,K+1,N,A] (the lag's hidden gradient), carry_sq
    [n_nets,B,T,K+1,N] (its squared norm) to produce; ``out``: optional dict of destination views for some of them (first four dims
    strided, inside their storage); ``scratch``: optional float32 buffer of at least ``gat_saliency_trace_scratch_floats`` floats;
    ``targets_dev``: optional int32 device tensor already holding ``targets`` (a caller that launches the same list many times uploads
    it once; the host list is still what the entry point checks).  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, keep = gat_saliency_trace_args(arena, saved, steps, v, targets, lags, gate_through, want, out, scratch, targets_dev)
    _launch("gat_saliency_trace_kernel", lambda: lib.call("iplan_gat_saliency_trace", a, L.current_stream(v.device)))
    res["_keep"] = keep
    return res


def gat_saliency_trace_args(arena, saved, steps, v, targets, lags=0, gate_through=True, want=("input_grad",), out=None, scratch=None,
                            targets_dev=None):
    """The descriptor of a ``gat_saliency_trace`` launch, its output tensors and what must stay alive until the launch has been
    queued, checked but not launched: (IplanGatSaliencyTraceArgs, dict, list)."""
    fa = saved["_args"]
    n_nets, rows, N, d0, d1 = fa.n_nets, fa.B, fa.N, fa.d0, fa.d1
    R, K = int(steps), int(lags)
    assert R >= 1 and rows % R == 0, (rows, R)
    B = rows // R
    A, D, n_src = 32, d0 + d1, 2 if d1 > 0 else 1
    dev = v.device
    want = tuple(want)
    assert want and all(k in GAT_SALIENCY_TRACE_OUTPUTS for k in want), want
    assert fa.params == arena.data.data_ptr(), "saved belongs to another arena"
    assert K >= 0, K
    targets = [int(t) for t in targets]
    T = len(targets)
    assert T >= 1 and all(0 <= t < R for t in targets), (targets, R)
    a = L.GatSaliencyTraceArgs()
    a.fwd = fa
    a.B, a.R, a.T, a.K = B, R, T, K
    t_host = (C.c_int32 * T)(*targets)
    if targets_dev is None:
        t_dev = torch.tensor(targets, dtype=torch.int32, device=dev)
    else:
        t_dev = targets_dev
        assert t_dev.shape == (T,) and t_dev.dtype == torch.int32 and t_dev.is_contiguous() and t_dev.device == dev, (t_dev.shape, t_dev.dtype)
    a.targets, a.targets_host = t_dev.data_ptr(), C.cast(t_host, C.c_void_p)
    assert v.shape == (n_nets, B, T, N, A) and v.dtype == torch.float32, (v.shape, v.dtype)
    a.v = v.data_ptr()
    a.v_s_net, a.v_s_b, a.v_s_t = _nbs_strides(v, N * A, "v")
    a.gate_through = 1 if gate_through else 0
    keep = [saved, v, t_host, t_dev]
    if gate_through:
        need = gat_saliency_trace_scratch_floats(n_nets, B, T, N)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.float32, device=dev)
        assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= need and scratch.device == dev, (scratch.numel(), need)
        a.scratch, a.scratch_floats = scratch.data_ptr(), scratch.numel()
        keep.append(scratch)
    res = {}
    inner = {"grad": (N, N, D), "pair_gl1": (N, N, n_src), "pair_gxi": (N, N, n_src), "input_grad": (N, D), "carry": (N, A), "carry_sq": (N,)}
    pre = {"grad": "grad", "input_grad": "ig", "carry": "carry", "carry_sq": "csq"}
    pair = None
    for k in want:
        t, *s = _dest_nbjs(out, res, k, (n_nets, B, T, K + 1), inner[k], dev)
        setattr(a, k, t.data_ptr())
        if k in pre:
            for name, x in zip(("net", "b", "t", "k"), s):
                setattr(a, f"{pre[k]}_s_{name}", x)
        else:
            assert pair is None or pair == tuple(s), "pair_gl1 and pair_gxi share their strides"
            pair = tuple(s)
            a.pair_s_net, a.pair_s_b, a.pair_s_t, a.pair_s_k = s
    return a, res, keep


_FUSED_SYNC = {}


def _fused_sync(dev):
    """the 3 counters of iplan_gat_enc_ac_fwd, private to (device, current stream)"""
    key = (str(dev), L.current_stream(dev))
    buf = _FUSED_SYNC.get(key)
    if buf is None:
        buf = _FUSED_SYNC[key] = torch.zeros(4, dtype=torch.int32, device=dev)
    return buf


def fused_sync_error():
    """True if any fused rollout launch gave up waiting for its producers (reads the device: tests / end of a rollout only)"""
    return any(int(b[2]) != 0 for b in _FUSED_SYNC.values())


def check_fused_sync():
    """Raise if a fused vector-step launch ran its action selection on stale latents (its wait hit the poll limit -- a scene or
    encoder workgroup never reported).  One 4-byte read-back per stream that ever ran a fused launch: call it where the host
    synchronises anyway (end of an episode / a training cycle)."""
    if fused_sync_error():
        for b in _FUSED_SYNC.values():                       # (a producer that reports after the give-up would leave the counters off by
            b.zero_()                                        #  one for every later launch: start the next one from a clean state)
        raise L.IplanError("iplan_gat_enc_ac_fwd: an action selection gave up waiting for the latent updates of its launch "
                           "(sync[2] != 0); the episode's actions from that step on are not valid")


def enc_forward(arena, x, h0, prev_latent, coef, Z, out_lat=None, out_h=None, lib=None, launch=True):
    """EncoderRNN + soft update for all nets.  x [n_nets,B,N,L,d] (any strides as long as the last dim is
    contiguous: a sliding window over a time-major observation log is read in place), h0 [n_nets,B,N,R],
    prev_latent [n_nets,B,N,Z] or None (first two dims may be strided views).  ``out_lat`` / ``out_h``:
    optional destinations of the same logical shapes (e.g. views into the episode buffer).
    Returns (latent [n_nets,B,N,Z], hL [n_nets,B,N,R])."""
    lib = _lib(lib)
    n_nets, B, N, Lw, d = x.shape
    R = h0.shape[-1]
    dev = x.device
    a = L.EncFwdArgs()
    a.n_nets, a.B, a.N, a.L, a.d, a.Z = n_nets, B, N, Lw, d, Z
    assert x.dtype == torch.float32 and x.stride(4) == 1
    a.x = x.data_ptr()
    a.x_s_net, a.x_s_b, a.x_s_i, a.x_s_t = x.stride(0), x.stride(1), x.stride(2), x.stride(3)
    a.h0 = h0.data_ptr()
    a.h0_s_net, a.h0_s_b = _nb_strides(h0, N * R)
    hL = out_h if out_h is not None else torch.empty(n_nets, B, N, R, dtype=torch.float32, device=dev)
    a.hL = hL.data_ptr()
    a.hL_s_net, a.hL_s_b = _nb_strides(hL, N * R)
    if prev_latent is not None:
        a.prev_latent = prev_latent.data_ptr()
        a.pl_s_net, a.pl_s_b = _nb_strides(prev_latent, N * Z)
    lat = out_lat if out_lat is not None else torch.empty(n_nets, B, N, Z, dtype=torch.float32, device=dev)
    a.latent_out = lat.data_ptr()
    a.lo_s_net, a.lo_s_b = _nb_strides(lat, N * Z)
    a.one_minus_c = 1.0 - coef
    a.c = coef
    a.params = arena.data.data_ptr()
    a.params_s_net = arena.net_stride
    for i, k in enumerate(L.ENC_PARAM_ORDER):
        a.off[i] = arena.off(k)
    if not launch:                                           # the caller hands ``args`` to gat_forward(fuse_enc=...)
        return lat, hL, dict(args=a, keep=(x, h0, prev_latent, lat, hL))
    lib.call("iplan_enc_fwd", a, L.current_stream(dev))
    return lat, hL


class AcFeatureSpec:
    """Where the actor/critic input row comes from (DcntrlMAC._build_inputs[_ippo] fused into the
    kernel).  ``sources``: up to three (tensor, width, s_net, s_row) per-entity fields; tensors are
    only referenced (kept alive) -- the kernel reads them in place."""

    def __init__(self, N, sources, n_actions=0, last_action=None, la_strides=(0, 0), n_id=0, T=1, T_phys=1):
        """last_action: int32 (or int64, read in place) tensor of hot indices (-1 = all zeros), or None."""
        self.N, self.sources, self.n_actions = N, sources, n_actions
        self.last_action, self.la_strides, self.n_id, self.T, self.T_phys = last_action, la_strides, n_id, T, T_phys

    @property
    def F(self):
        return self.N * sum(s[1] for s in self.sources) + self.n_actions + self.n_id

    def fill(self, f):
        f.N = self.N
        for k in range(3):
            if k < len(self.sources):
                t, w, s_net, s_row = self.sources[k]
                assert t.dtype == torch.float32
                f.w[k], f.src[k], f.s_net[k], f.s_row[k] = w, t.data_ptr(), s_net, s_row
            else:
                f.w[k], f.src[k], f.s_net[k], f.s_row[k] = 0, None, 0, 0
        f.n_actions = self.n_actions
        if self.last_action is not None:
            if self.last_action.dtype == torch.int64:
                f.last_action64 = self.last_action.data_ptr()
                f.la64_s_net, f.la64_s_row = self.la_strides
            else:
                assert self.last_action.dtype == torch.int32
                f.last_action = self.last_action.data_ptr()
                f.la_s_net, f.la_s_row = self.la_strides
        f.n_id = self.n_id
        f.T, f.T_phys = self.T, self.T_phys


def _fill_acnet(dst, arena, order, n_out):
    dst.params = arena.data.data_ptr()
    dst.params_s_net = arena.net_stride
    for i, k in enumerate(order):
        dst.off[i] = arena.off(k)
    dst.n_out = n_out


def ac_forward(actor_arena, critic_arena, which, spec, rows, n_agents, h_actor=None, h_critic=None,
               h_strides=(0, 0), avail=None, avail_strides=(0, 0), mode=0, q_noise=None, actions_in=None,
               act_strides=(0, 0), n_actions=5, ksplit=None, save=False, want_probs=False, want_entropy=False,
               want_h=True, h_out=None, actions_out=None, onehot_out=None, ln_stats=None, ln_stats_mode=0, phase_clocks=None,
               packed=None, xhat=None, lib=None, launch=True):
    """Fused actor (which=0) / critic (1) / both (2) forward for all agents.
    ``launch=False`` (rollout shape only): everything is set up but nothing is enqueued -- the returned dict goes to
    ``gat_forward(fuse_ac=...)``, whose launch runs this action selection behind the latent updates it depends on.
    Returns a dict with the requested outputs, each laid out [n_agents, rows, ...].
    Optional in-place destinations (rollout: write straight into the episode buffer):
      h_out = (actor_tensor, critic_tensor, (s_net, s_row));  actions_out = (int64 tensor, (s_net, s_row));
      onehot_out = (float tensor, (s_net, s_row)).
    ln_stats [n_agents, n_physical_rows, 2] with ln_stats_mode 1 (compute + store) / 2 (re-use).
    xhat: ``ac_xhat_pack(...)`` of the same (spec, rows) -- which = 2 only: fc1 runs as the split-bf16 contraction over the
    packed rows (iplan_ac_fc1_split_fwd) and this launch is the 64-wide tail; ``ac_backward`` then takes the matching path."""
    lib = _lib(lib)
    dev = (actor_arena if which != 1 else critic_arena).data.device
    a = L.AcFwdArgs()
    a.n_agents, a.rows, a.which = n_agents, rows, which
    a.ksplit = ksplit if ksplit is not None else (8 if rows <= 512 else 1)
    a.act_tanh = int(bool(getattr(actor_arena if which != 1 else critic_arena, "act_tanh", False)))
    if which == 2:                                            # one flag for both nets of the launch (and of its backward tail)
        assert bool(getattr(actor_arena, "act_tanh", False)) == bool(getattr(critic_arena, "act_tanh", False)), \
            "actor and critic of one fused launch must use the same trunk activation (args.use_ReLU)"
    spec.fill(a.feat)
    out = {}
    f32 = dict(dtype=torch.float32, device=dev)
    if which != 1:
        _fill_acnet(a.actor, actor_arena, L.ACTOR_PARAM_ORDER, n_actions)
        a.h_actor = h_actor.data_ptr()
        if h_out is not None:
            a.h_actor_out = h_out[0].data_ptr()
        elif want_h:
            out["h_actor"] = torch.empty(n_agents, rows, L.AC_HIDDEN, **f32)
            a.h_actor_out = out["h_actor"].data_ptr()
        if avail is not None:
            assert avail.dtype == torch.int32
            a.avail = avail.data_ptr()
            a.av_s_net, a.av_s_row = avail_strides
        a.mode = mode
        if mode == 1:
            assert q_noise.shape == (n_agents, rows, n_actions) and q_noise.is_contiguous()
            a.q_noise = q_noise.data_ptr()
        if mode == 2:
            assert actions_in.dtype == torch.int64
            a.actions_in = actions_in.data_ptr()
            a.act_s_net, a.act_s_row = act_strides
        elif actions_out is not None:
            assert actions_out[0].dtype == torch.int64
            a.actions_out = actions_out[0].data_ptr()
            a.ao_s_net, a.ao_s_row = actions_out[1]
        else:
            out["actions"] = torch.empty(n_agents, rows, dtype=torch.int64, device=dev)
            a.actions_out = out["actions"].data_ptr()
        if onehot_out is not None and mode != 2:
            assert onehot_out[0].dtype == torch.float32
            a.onehot_out = onehot_out[0].data_ptr()
            a.oh_s_net, a.oh_s_row = onehot_out[1]
        out["logp"] = torch.empty(n_agents, rows, **f32)
        a.logp = out["logp"].data_ptr()
        if want_entropy:
            out["entropy"] = torch.empty(n_agents, rows, **f32)
            a.entropy = out["entropy"].data_ptr()
        if want_probs:
            out["probs"] = torch.empty(n_agents, rows, n_actions, **f32)
            a.probs = out["probs"].data_ptr()
    if which != 0:
        _fill_acnet(a.critic, critic_arena, L.CRITIC_PARAM_ORDER, 1)
        a.h_critic = h_critic.data_ptr()
        if h_out is not None:
            a.h_critic_out = h_out[1].data_ptr()
        elif want_h:
            out["h_critic"] = torch.empty(n_agents, rows, L.AC_HIDDEN, **f32)
            a.h_critic_out = out["h_critic"].data_ptr()
        out["values"] = torch.empty(n_agents, rows, **f32)
        a.values = out["values"].data_ptr()
    a.hs_net, a.hs_row = h_strides
    if h_out is not None:
        a.ho_s_net, a.ho_s_row = h_out[2]
    if ln_stats is not None and ln_stats_mode:
        assert (ln_stats.dtype == torch.float32 and ln_stats.shape[0] == n_agents and ln_stats.shape[2] == 2
                and ln_stats.stride(2) == 1 and ln_stats.stride(1) == 2)          # rows contiguous (a row range of a larger buffer is fine)
        a.ln_stats, a.ln_stats_s_net, a.ln_stats_mode = ln_stats.data_ptr(), ln_stats.stride(0), ln_stats_mode
    if phase_clocks is not None:
        a.phase_clocks = phase_clocks.data_ptr()
    if packed is not None:                                 # Fc1Pack.get(): fragment-major fc1 operands of both arenas
        pa, pc = packed
        if a.ksplit > 1 and a.ln_stats_mode == 0:           # the folded form reads W gamma / W beta from the pack
            assert getattr(packed, "fold", False), "rollout-shaped launch needs Fc1Pack.get(spec, fold=True)"
        if which != 1:
            a.packed_actor, a.packed_s_net = pa.data_ptr(), pa.stride(0)
        if which != 0:
            a.packed_critic, a.packed_s_net = pc.data_ptr(), pc.stride(0)
    if save:
        out["saved"] = torch.empty(2, n_agents, rows, L.AC_SAVE_FLOATS, **f32)
        a.saved = out["saved"].data_ptr()
    ks_bufs = None
    units = ((rows + 15) // 16) * n_agents * (2 if which == 2 else 1)
    # rollout shape: the F-wide contraction of every (row tile, net) unit over kw workgroups (include/iplan_hip.h: ksplit_wg)
    # while the launch is far from filling the 256 CUs: 4 up to 40 units (config 3: 20), 2 up to 96, off beyond
    kw = int(os.environ.get("IPLAN_AC_KSPLIT_WG", "0")) or (4 if units <= 40 else (2 if units <= 96 else 1))
    if (kw > 1 and a.ksplit == 8 and not save and a.ln_stats_mode == 0 and packed is not None and getattr(packed, "fold", False)):
        key = (str(dev), L.current_stream(dev), units, kw)
        ks_bufs = _KSPLIT_BUFS.get(key)
        if ks_bufs is None:
            ks_bufs = _KSPLIT_BUFS[key] = (torch.empty(units * kw * L.AC_KS_SLOT_FLOATS, **f32),
                                           torch.zeros(units, dtype=torch.int32, device=dev))
        a.ksplit_wg, a.ks_scratch, a.ks_count = kw, ks_bufs[0].data_ptr(), ks_bufs[1].data_ptr()
    z1 = None
    if xhat is not None:
        assert which == 2 and a.ksplit == 1 and ln_stats_mode == 2 and xhat["rows"] == rows and xhat["n_agents"] == n_agents
        s = L.AcFc1SplitArgs()
        s.n_agents, s.rows = n_agents, rows
        spec.fill(s.feat)
        s.actor, s.critic = a.actor, a.critic
        KS = (xhat["KT"] + 1) // 2
        ws = workspace(dev, n_agents * KS * 6144 + 2 * n_agents * L.AC_HIDDEN, "fc1_split")
        kparts = int(lib.c.iplan_ac_fc1_split_parts(n_agents, rows))           # > 1: small batches, the K loop over several workgroups
        z1 = torch.empty(kparts, 2, n_agents, rows, L.AC_HIDDEN, **f32)
        s.kparts, a.fc1_pre_parts = kparts, kparts
        s.xf, s.wsplit, s.wbeta, s.z1 = xhat["xf"].data_ptr(), ws.data_ptr(), ws.data_ptr() + 4 * n_agents * KS * 6144, z1.data_ptr()
        # algorithmic work of the launch: 2 FLOP per (row, feature, output) of both nets
        _launch("ac_fc1_split_fwd", lambda: lib.call("iplan_ac_fc1_split_fwd", s, L.current_stream(dev)),
                work=2.0 * n_agents * rows * spec.F * 2 * L.AC_HIDDEN)
        a.fc1_pre = z1.data_ptr()
        out["_xhat"] = xhat
    if launch:
        _launch("ac_fwd_kernel:train" if save else ("ac_fwd_kernel:rollout" if rows <= 512 else "ac_fwd_kernel:infer"),
                lambda: lib.call("iplan_ac_fwd", a, L.current_stream(dev)))
    else:
        assert a.ksplit == 8 and not save and xhat is None and a.ln_stats_mode == 0, "launch=False is for the rollout-shaped forward"
    out["_args"] = a
    out["_keep"] = (spec, h_actor, h_critic, avail, q_noise, actions_in, h_out, actions_out, onehot_out, ln_stats, packed, z1, xhat, ks_bufs)
    return out


POLICY_TRACE_OUTPUTS = ("probs", "entropy", "greedy", "logp", "values", "h_actor", "h_critic")


def _inside(t, reach, what):
    """the last element a kernel can touch through ``t.data_ptr()``, ``reach`` elements past it, lies inside t's storage"""
    assert 0 <= reach <= _room(t), (what, "reaches outside its storage", reach, _room(t))


def _dest(out, res, k, shape, dtype, dev, fresh=torch.empty):
    """``out[k]`` if the caller gave one, else a ``fresh`` tensor: contiguous, of exactly ``shape`` and ``dtype`` on ``dev``; entered
    into ``res`` -> its address"""
    t = None if out is None else out.get(k)
    if t is None:
        t = fresh(*shape, dtype=dtype, device=dev)
    assert t.shape == tuple(shape) and t.dtype == dtype and t.device == dev and t.is_contiguous(), (k, t.shape, t.dtype)
    res[k] = t
    return t.data_ptr()


def _ac_rows(a, actor_arena, critic_arena, which, spec, E, S, n_agents):
    """What every launch over E x S recorded rows of the actors / critics checks and enters into its descriptor ``a``: ``which``, the
    sizes, one trunk activation for both arenas, ``spec`` (T = S) with every feature source and the last action inside their storage
    -> (the device, the largest physical row)"""
    assert which in (0, 1, 2) and E >= 1 and S >= 1 and n_agents >= 1, (which, E, S, n_agents)
    arena0 = actor_arena if which != 1 else critic_arena
    dev = arena0.data.device
    a.n_agents, a.E, a.S, a.which = n_agents, E, S, which
    a.act_tanh = int(bool(getattr(arena0, "act_tanh", False)))
    if which == 2:
        assert bool(getattr(actor_arena, "act_tanh", False)) == bool(getattr(critic_arena, "act_tanh", False)), \
            "actor and critic of one launch must use the same trunk activation (args.use_ReLU)"
    assert spec.T == S and spec.T_phys >= S, (spec.T, spec.T_phys, S)
    spec.fill(a.feat)
    last_row = (E - 1) * spec.T_phys + S - 1                         # the largest physical row
    for t, w, s_net, s_row in spec.sources:
        assert t.device == dev and min(s_net, s_row) >= 0
        _inside(t, (n_agents - 1) * s_net + last_row * s_row + spec.N * w, "feature source")
    if spec.last_action is not None and spec.n_actions > 0:
        assert spec.last_action.device == dev and min(spec.la_strides) >= 0
        _inside(spec.last_action, (n_agents - 1) * spec.la_strides[0] + last_row * spec.la_strides[1] + 1, "last_action")
    return dev, last_row


def _ac_packed(a, which, packed):
    """``packed``: Fc1Pack.get(spec) or None; the fragment part (and gamma) is all these kernels read"""
    if packed is not None:
        pa, pc = packed
        if which != 1:
            a.packed_actor, a.packed_s_net = pa.data_ptr(), pa.stride(0)
        if which != 0:
            a.packed_critic, a.packed_s_net = pc.data_ptr(), pc.stride(0)


def _job_list(a, jobs, N, dev):
    """``jobs``: J >= 1 entity indices in [0, N), or -1 for "nothing knocked", entered into the descriptor ``a`` (J, jobs, jobs_host) as
    the device copy the kernel reads and the host copy the entry point checks -> both copies, to be kept alive"""
    jobs = [int(j) for j in jobs]
    J = len(jobs)
    assert J >= 1 and all(-1 <= j < N for j in jobs), (jobs, N)
    j_host = (C.c_int32 * J)(*jobs)
    j_dev = torch.tensor(jobs, dtype=torch.int32, device=dev)
    a.J, a.jobs, a.jobs_host = J, j_dev.data_ptr(), C.cast(j_host, C.c_void_p)
    return j_host, j_dev


def _enc_rows(a, enc_arena, hist, L_win, Z, coef):
    """What every launch over the behaviour encoder's chain checks and enters into its descriptor ``a``: hist [n_nets, E, T, N, d] with
    contiguous (N, d) rows, the sizes, the history's strides, ``coef``, the encoder's arena and its offsets -> hist's shape"""
    n_nets, E, T, N, d = hist.shape
    assert hist.dtype == torch.float32 and hist.stride(4) == 1 and hist.stride(3) == d
    a.n_nets, a.E, a.N, a.T, a.L, a.d, a.Z = n_nets, E, N, T, L_win, d, Z
    a.hist, a.h_s_net, a.h_s_e, a.h_s_t = hist.data_ptr(), hist.stride(0), hist.stride(1), hist.stride(2)
    a.coef = coef
    a.enc_params, a.enc_s_net = enc_arena.data.data_ptr(), enc_arena.net_stride
    for i, k in enumerate(L.ENC_PARAM_ORDER):
        a.enc_off[i] = enc_arena.off(k)
    return n_nets, E, T, N, d


def _index_list(a, name, idx, dev):
    """``idx`` as ints, entered into the descriptor ``a`` as ``name`` (the device copy the kernel reads; null for an empty list) and
    ``name``_host (the host copy the entry point checks) -> (the ints, both copies, to be kept alive)"""
    idx = [int(i) for i in idx]
    i_host = (C.c_int32 * max(len(idx), 1))(*idx)
    i_dev = torch.tensor(idx, dtype=torch.int32, device=dev) if idx else None
    setattr(a, name, L.ptr(i_dev))
    setattr(a, name + "_host", C.cast(i_host, C.c_void_p))
    return idx, i_host, i_dev


def _per_source(seq, n_src, what):
    """``seq`` (None: nothing) as one entry per source of the rows; it may be shorter, and longer only with nothing past the end"""
    seq = (None,) * n_src if seq is None else tuple(seq)
    assert all(v is None or v is False for v in seq[n_src:]), (what, "names a source the rows do not have", n_src)
    return seq[:n_src] + (None,) * (n_src - len(seq))


def _knock_baseline(a, spec, knock, baseline, dev):
    """Per source of ``spec``, into the knock-out descriptor ``a``: the ``knock`` flags (None: every source) and the ``baseline`` rows
    [w] or None (zeros); neither may name an absent source -> the rows, to be kept alive"""
    n_src = len(spec.sources)
    knock = (True,) * n_src if knock is None else _per_source(knock, n_src, "knock")
    baseline = _per_source(baseline, n_src, "baseline")
    for k, (_, w, _, _) in enumerate(spec.sources):
        a.knock[k] = int(bool(knock[k]))
        row = baseline[k]
        assert w > 0 or not (a.knock[k] or row is not None), ("source", k, "is absent")
        if row is not None:
            assert row.shape == (w,) and row.dtype == torch.float32 and row.is_contiguous() and row.device == dev, ("baseline", k, tuple(row.shape), w)
            a.baseline[k] = row.data_ptr()
    return baseline


def _pair_dests(a, which, want, dest, pair, n_actions):
    """the per-(row, job) destinations, ``pair`` = their shape, that both policy knock-out descriptors name alike"""
    if which != 1:
        for k, inner, dtype in (("kl", (), torch.float32), ("dlogp", (), torch.float32), ("greedy_ko", (), torch.int64),
                                ("probs_ko", (n_actions,), torch.float32), ("logp_ko", (), torch.float32)):
            if k in want:
                setattr(a, k, dest(k, pair + inner, dtype))
    if which != 0:
        for k in ("dvalue", "values_ko"):
            if k in want:
                setattr(a, k, dest(k, pair))


def _chain_operands(a, which, n_agents, E, last_row, dev, n_actions, hidden0_actor, hidden0_critic, h_strides, avail, avail_strides, actions_in,
                    act_strides, what="actions_in"):
    """What a walk over E chains reads beside its rows, into the IplanAcTraceArgs ``a``: hidden0_* [.., 64] by (net, chain) (None:
    zeros) and, by physical row, the actors' avail int32 [.., n_actions] and actions_in int64, each checked to lie inside its storage"""
    for net, h0, key in ((0, hidden0_actor, "actor"), (1, hidden0_critic, "critic")):
        if which == 1 - net or h0 is None:
            continue
        assert h0.dtype == torch.float32 and h0.device == dev and min(h_strides) >= 0
        _inside(h0, (n_agents - 1) * h_strides[0] + (E - 1) * h_strides[1] + L.AC_HIDDEN, "hidden0_" + key)
        setattr(a, "hidden0_" + key, h0.data_ptr())
    a.h0_s_net, a.h0_s_chain = h_strides
    if which == 1:
        return
    if avail is not None:
        assert avail.dtype == torch.int32 and avail.device == dev and min(avail_strides) >= 0
        _inside(avail, (n_agents - 1) * avail_strides[0] + last_row * avail_strides[1] + n_actions, "avail")
        a.avail = avail.data_ptr()
        a.av_s_net, a.av_s_row = avail_strides
    if actions_in is not None:
        assert actions_in.dtype == torch.int64 and actions_in.device == dev and min(act_strides) >= 0
        _inside(actions_in, (n_agents - 1) * act_strides[0] + last_row * act_strides[1] + 1, what)
        a.actions_in = actions_in.data_ptr()
        a.act_s_net, a.act_s_row = act_strides


def policy_trace(actor_arena, critic_arena, which, spec, E, S, n_agents, hidden0_actor=None, hidden0_critic=None, h_strides=(0, 0),
                 avail=None, avail_strides=(0, 0), actions_in=None, act_strides=(0, 0), n_actions=5,
                 want=("probs", "entropy", "greedy", "logp", "values"), packed=None, out=None, lib=None):
    """R_Actor (which=0) / R_Critic (1) / both (2) of every agent walked over the S consecutive steps of E recorded chains
    (iplan_ac_trace: a row-parallel trunk kernel, then a walk that carries the GRU state), forward only.  ``spec``: the rows'
    features as for ``ac_forward`` with T = S -- row (e, s) at physical row e * T_phys + s, its last action teacher-forced from
    ``spec.last_action`` (-1: zeros).  hidden0_* [.., 64] at net * h_strides[0] + e * h_strides[1] (None: zeros); avail int32 and
    actions_in int64 are addressed by physical row with their (s_net, s_row) strides.  ``want``: which of probs [nA,E,S,n_actions],
    entropy / logp / values [nA,E,S], greedy [nA,E,S] int64, h_actor / h_critic [nA,E,S,64] (the state after every step) to
    produce; ``out``: optional dict of contiguous destinations for some of them.  The state after the last step is always
    returned as h_last_actor / h_last_critic [nA,E,64].  ``packed``: Fc1Pack.get(spec) or None (same bits).  Everything the
    kernels will read is bounds-checked here, on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, _keep = policy_trace_args(actor_arena, critic_arena, which, spec, E, S, n_agents, hidden0_actor, hidden0_critic, h_strides,
                                      avail, avail_strides, actions_in, act_strides, n_actions, want, packed, out)
    dev = (actor_arena if which != 1 else critic_arena).data.device
    nets = n_agents * (2 if which == 2 else 1)
    _launch("ac_trace", lambda: lib.call("iplan_ac_trace", a, L.current_stream(dev)),
            work=2.0 * nets * E * S * L.AC_HIDDEN * (spec.F + 7 * L.AC_HIDDEN))
    return res


def policy_trace_args(actor_arena, critic_arena, which, spec, E, S, n_agents, hidden0_actor=None, hidden0_critic=None, h_strides=(0, 0),
                      avail=None, avail_strides=(0, 0), actions_in=None, act_strides=(0, 0), n_actions=5,
                      want=("probs", "entropy", "greedy", "logp", "values"), packed=None, out=None):
    """The descriptor of a ``policy_trace`` launch, its output tensors and the operands to keep alive until the launch has been
    queued, checked but not launched: (IplanAcTraceArgs, dict, tuple)."""
    want = tuple(want)
    assert all(k in POLICY_TRACE_OUTPUTS for k in want), want
    M = L.AC_HIDDEN
    a = L.AcTraceArgs()
    dev, last_row = _ac_rows(a, actor_arena, critic_arena, which, spec, E, S, n_agents)
    res = {}

    def dest(k, shape, dtype=torch.float32):
        return _dest(out, res, k, shape, dtype, dev)

    _chain_operands(a, which, n_agents, E, last_row, dev, n_actions, hidden0_actor, hidden0_critic, h_strides, avail, avail_strides, actions_in,
                    act_strides)
    for net, key in ((0, "actor"), (1, "critic")):
        if which == 1 - net:
            continue
        setattr(a, "h_last_" + key, dest("h_last_" + key, (n_agents, E, M)))
        if "h_" + key in want:
            setattr(a, "h_all_" + key, dest("h_" + key, (n_agents, E, S, M)))
    if which != 1:
        _fill_acnet(a.actor, actor_arena, L.ACTOR_PARAM_ORDER, n_actions)
        if "probs" in want:
            a.probs = dest("probs", (n_agents, E, S, n_actions))
        if "entropy" in want:
            a.entropy = dest("entropy", (n_agents, E, S))
        if "greedy" in want:
            a.greedy = dest("greedy", (n_agents, E, S), torch.int64)
        if "logp" in want:
            a.logp = dest("logp", (n_agents, E, S))
    if which != 0:
        _fill_acnet(a.critic, critic_arena, L.CRITIC_PARAM_ORDER, 1)
        if "values" in want:
            a.values = dest("values", (n_agents, E, S))
    _ac_packed(a, which, packed)
    gi = workspace(dev, 2 * n_agents * E * S * L.AC_TRACE_GI, "ac_trace")
    a.gi = gi.data_ptr()
    return a, res, (spec, hidden0_actor, hidden0_critic, avail, actions_in, packed, gi)


SALIENCY_OUTPUTS = ("y", "entity", "input_grad", "act")


def saliency(actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor=None, h_critic=None, h_strides=(0, 0, 0), avail=None,
             avail_strides=(0, 0, 0), target=None, target_strides=(0, 0, 0), target_all=-1, n_actions=5, want=("y", "entity"), packed=None,
             out=None, lib=None):
    """Input gradients of R_Actor (which=0) / R_Critic (1) / both (2) of every agent on E x S independent rows (iplan_ac_saliency; include/
    iplan_hip.h: IplanAcSaliencyArgs): d log pi(a* | x) / d x and d V / d x with the row's GRU state GIVEN and held constant.  ``spec``:
    the rows' features as for ``policy_trace`` (T = S, row (e, s) at physical row e * T_phys + s).  h_actor / h_critic [.., 64], avail
    int32 [.., n_actions] and target int64 are addressed with their own (net, chain, step) strides; ``target`` None: ``target_all`` for
    every row; -1 = the row's greedy action.  ``want``: "y" (logp, values, target_action [nA,E,S]), "entity" (entity_actor /
    entity_critic [nA,E,S,N,n_src,2]: sum g x and sum |g| per entity and enabled source), "input_grad" (input_grad_* [nA,E,S,F], the
    reference's column order), "act" (act1_* / act2_* [nA,E,S,64], the trunk's post-activation tiles).  ``out``: optional dict of
    contiguous destinations.  ``packed``: Fc1Pack.get(spec) or None (same bits).  Everything the kernel will read is bounds-checked here,
    on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, _keep = saliency_args(actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor, h_critic, h_strides, avail, avail_strides,
                                  target, target_strides, target_all, n_actions, want, packed, out)
    dev = (actor_arena if which != 1 else critic_arena).data.device
    nets = n_agents * (2 if which == 2 else 1)
    _launch("ac_saliency", lambda: lib.call("iplan_ac_saliency", a, L.current_stream(dev)),
            work=2.0 * nets * E * S * L.AC_HIDDEN * (3 * spec.F + 14 * L.AC_HIDDEN))
    return res


def _saliency_rows(a, actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor, h_critic, h_strides, avail, avail_strides, target,
                   target_strides, target_all, n_actions):
    """What the launches over E x S rows with a GIVEN GRU state per row enter into their IplanAcSaliencyArgs ``a`` beside ``_ac_rows``:
    the states, the nets, avail and the target, each checked to lie inside its storage -> the device"""
    M = L.AC_HIDDEN
    dev, _ = _ac_rows(a, actor_arena, critic_arena, which, spec, E, S, n_agents)
    a.target_all = target_all

    def reach(strides, width):
        assert len(strides) == 3 and min(strides) >= 0, strides
        return (n_agents - 1) * strides[0] + (E - 1) * strides[1] + (S - 1) * strides[2] + width

    for net, h, key in ((0, h_actor, "actor"), (1, h_critic, "critic")):
        if which == 1 - net:
            continue
        assert h is not None and h.dtype == torch.float32 and h.device == dev, ("the GRU state of the " + key + "s is needed",)
        _inside(h, reach(h_strides, M), "h_" + key)
        setattr(a, "h_" + key, h.data_ptr())
    a.hs_net, a.hs_chain, a.hs_step = h_strides
    if which != 1:
        _fill_acnet(a.actor, actor_arena, L.ACTOR_PARAM_ORDER, n_actions)
        if avail is not None:
            assert avail.dtype == torch.int32 and avail.device == dev
            _inside(avail, reach(avail_strides, n_actions), "avail")
            a.avail = avail.data_ptr()
            a.av_s_net, a.av_s_chain, a.av_s_step = avail_strides
        if target is not None:
            assert target.dtype == torch.int64 and target.device == dev
            _inside(target, reach(target_strides, 1), "target")
            a.target = target.data_ptr()
            a.tg_s_net, a.tg_s_chain, a.tg_s_step = target_strides
    if which != 0:
        _fill_acnet(a.critic, critic_arena, L.CRITIC_PARAM_ORDER, 1)
    return dev


def _saliency_y(a, which, dest, n_agents, E, S):
    """logp, target_action and values [nA, E, S] of the selected nets as destinations of ``a``"""
    if which != 1:
        a.logp = dest("logp", (n_agents, E, S))
        a.target_out = dest("target_action", (n_agents, E, S), torch.int64)
    if which != 0:
        a.values = dest("values", (n_agents, E, S))


def saliency_args(actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor=None, h_critic=None, h_strides=(0, 0, 0), avail=None,
                  avail_strides=(0, 0, 0), target=None, target_strides=(0, 0, 0), target_all=-1, n_actions=5, want=("y", "entity"), packed=None,
                  out=None):
    """The descriptor of a ``saliency`` launch, its output tensors and the operands to keep alive until the launch has been queued,
    checked but not launched: (IplanAcSaliencyArgs, dict, tuple)."""
    want = tuple(want)
    assert want and all(k in SALIENCY_OUTPUTS for k in want), want
    M = L.AC_HIDDEN
    a = L.AcSaliencyArgs()
    dev = _saliency_rows(a, actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor, h_critic, h_strides, avail, avail_strides, target,
                         target_strides, target_all, n_actions)
    n_src = sum(1 for s in spec.sources if s[1] > 0)
    res = {}

    def dest(k, shape, dtype=torch.float32):
        return _dest(out, res, k, shape, dtype, dev)

    for net, key in ((0, "actor"), (1, "critic")):
        if which == 1 - net:
            continue
        if "entity" in want:
            setattr(a, "entity_" + key, dest("entity_" + key, (n_agents, E, S, spec.N, n_src, 2)))
        if "input_grad" in want:
            setattr(a, "input_grad_" + key, dest("input_grad_" + key, (n_agents, E, S, spec.F)))
        if "act" in want:
            setattr(a, "act1_" + key, dest("act1_" + key, (n_agents, E, S, M)))
            setattr(a, "act2_" + key, dest("act2_" + key, (n_agents, E, S, M)))
    if "y" in want:
        _saliency_y(a, which, dest, n_agents, E, S)
    _ac_packed(a, which, packed)
    return a, res, (spec, h_actor, h_critic, avail, target, packed)


POLICY_KNOCKOUT_OUTPUTS = ("base", "kl", "dlogp", "dvalue", "greedy_ko", "probs_ko", "logp_ko", "values_ko")
POLICY_KNOCKOUT_JOBS_PER_TILE = 15       # KO_JOBS of csrc/policy_knockout.hip: column 15 of every tile carries the row's base result


def policy_knockout(actor_arena, critic_arena, which, spec, E, S, n_agents, jobs, h_actor=None, h_critic=None, h_strides=(0, 0, 0), avail=None,
                    avail_strides=(0, 0, 0), target=None, target_strides=(0, 0, 0), target_all=-1, n_actions=5, knock=None, baseline=None,
                    override=None, want=("kl",), packed=None, out=None, lib=None):
    """R_Actor (which=0) / R_Critic (1) / both (2) of every agent on E x S recorded rows, run once per job with one entity's columns of
    the selected sources replaced as the features are gathered (iplan_ac_knockout; include/iplan_hip.h: IplanAcKnockoutArgs), forward
    only, the row's GRU state given and held.  ``spec``, h_*, avail, target, ``packed`` and their strides as for ``saliency``.
    ``jobs``: J entity indices in [0, N), or -1 for "nothing knocked" (duplicates allowed), shared by all rows.  Per source, in the
    order of ``spec.sources``: ``knock`` flags (None: every source), ``baseline`` rows [w] or None (zeros), ``override`` views
    [nA, E, S, J, N, w] or None -- any non-negative strides with the innermost axis contiguous, read in place; an overridden source is
    taken as given and not knocked as well.  ``want``: "base" (logp, values, target_action, greedy [nA,E,S] and probs [nA,E,S,n_actions]
    of the rows with nothing knocked) and, [nA,E,S,J] each, kl = KL(pi_base || pi_ko), dlogp, dvalue, greedy_ko (int64), logp_ko,
    values_ko, probs_ko [.., n_actions]; those the selected nets do not provide are left out.  ``out``: optional dict of contiguous
    destinations.  Everything the kernel will read is bounds-checked here, on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, _keep = policy_knockout_args(actor_arena, critic_arena, which, spec, E, S, n_agents, jobs, h_actor, h_critic, h_strides, avail,
                                         avail_strides, target, target_strides, target_all, n_actions, knock, baseline, override, want, packed, out)
    dev = (actor_arena if which != 1 else critic_arena).data.device
    nets = n_agents * (2 if which == 2 else 1)
    cols = 16 * ((a.J + POLICY_KNOCKOUT_JOBS_PER_TILE - 1) // POLICY_KNOCKOUT_JOBS_PER_TILE)
    _launch("ac_knockout", lambda: lib.call("iplan_ac_knockout", a, L.current_stream(dev)),
            work=2.0 * nets * E * S * cols * L.AC_HIDDEN * (spec.F + 8 * L.AC_HIDDEN))
    return res


def policy_knockout_args(actor_arena, critic_arena, which, spec, E, S, n_agents, jobs, h_actor=None, h_critic=None, h_strides=(0, 0, 0), avail=None,
                         avail_strides=(0, 0, 0), target=None, target_strides=(0, 0, 0), target_all=-1, n_actions=5, knock=None, baseline=None,
                         override=None, want=("kl",), packed=None, out=None):
    """The descriptor of a ``policy_knockout`` launch, its output tensors and the operands to keep alive until the launch has been
    queued, checked but not launched: (IplanAcKnockoutArgs, dict, tuple)."""
    want = tuple(want)
    assert want and all(k in POLICY_KNOCKOUT_OUTPUTS for k in want), want
    N = spec.N
    # the rows, the states, avail and target as saliency describes them; its "y" outputs receive the base result
    a = L.AcKnockoutArgs()
    dev = _saliency_rows(a.base, actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor, h_critic, h_strides, avail, avail_strides, target,
                         target_strides, target_all, n_actions)
    _ac_packed(a.base, which, packed)
    res = {}

    def dest(k, shape, dtype=torch.float32):
        return _dest(out, res, k, shape, dtype, dev)

    if "base" in want:
        _saliency_y(a.base, which, dest, n_agents, E, S)
    keep = (spec, h_actor, h_critic, avail, target, packed) + _job_list(a, jobs, N, dev) + _knock_baseline(a, spec, knock, baseline, dev)
    J = a.J
    override = _per_source(override, len(spec.sources), "override")
    for k, (_, w, _, _) in enumerate(spec.sources):
        ov = override[k]
        if ov is not None:
            assert w > 0, ("source", k, "is absent")
            assert ov.shape == (n_agents, E, S, J, N, w) and ov.dtype == torch.float32 and ov.device == dev, ("override", k, tuple(ov.shape))
            st = ov.stride()
            assert min(st) >= 0 and (st[5] == 1 or w == 1), ("override", k, "negative stride or a strided innermost axis", st)
            _inside(ov, sum((n - 1) * s for n, s in zip(ov.shape[:5], st[:5])) + w, "override")
            a.override_src[k] = ov.data_ptr()
            a.ov_s_net[k], a.ov_s_chain[k], a.ov_s_step[k], a.ov_s_job[k], a.ov_s_ent[k] = st[:5]
    if which != 1 and "base" in want:
        a.probs_base = dest("probs", (n_agents, E, S, n_actions))
        a.greedy_base = dest("greedy", (n_agents, E, S), torch.int64)
    _pair_dests(a, which, want, dest, (n_agents, E, S, J), n_actions)
    assert res, ("nothing of", want, "is provided by the selected nets")
    return a, res, keep + override


POLICY_KNOCKOUT_TRACE_OUTPUTS = ("base", "kl", "dlogp", "dvalue", "greedy_ko", "shift_sq", "probs_ko", "logp_ko", "values_ko", "h_ko", "logp_all_ko",
                                 "gi_ko")


def policy_knockout_trace_gi_floats(which, n_agents, E, H, D, J, override=False):
    """floats of the two gi workspaces of one ``policy_knockout_trace`` launch: the rows' base gi [2, nA, E * H, 192] (not needed when
    D = H) and the knocked columns' gi_ko [2, nA, E, D, ceil(J / 15), 16, 192]; with ``override`` (a source has a per-job override) the
    H-deep gi_ko [2, nA, E, H, ceil(J / 15), 16, 192] alone"""
    JT = (J + POLICY_KNOCKOUT_JOBS_PER_TILE - 1) // POLICY_KNOCKOUT_JOBS_PER_TILE
    if override:
        return 2 * n_agents * E * L.AC_TRACE_GI * H * JT * 16
    return 2 * n_agents * E * L.AC_TRACE_GI * ((H if D < H else 0) + D * JT * 16)


def _chain_overrides(c, spec, n_agents, E, H, J, dev, override, override_base):
    """the per-job and base overrides of ``policy_knockout_trace`` into IplanAcKnockoutChainArgs, per source in ``spec.sources`` order:
    views [nA, E, H, J, N, w] and [nA, E, H, N, w], any non-negative strides with the innermost axis contiguous, bounds-checked"""
    N = spec.N
    for k, (_, w, _, _) in enumerate(spec.sources):
        for ov, shape, what in ((override[k], (n_agents, E, H, J, N, w), "override"), (override_base[k], (n_agents, E, H, N, w), "override_base")):
            if ov is None:
                continue
            assert w > 0, ("source", k, "is absent")
            assert ov.shape == shape and ov.dtype == torch.float32 and ov.device == dev, (what, k, tuple(ov.shape), shape)
            st = ov.stride()
            assert min(st) >= 0 and (st[-1] == 1 or w == 1), (what, k, "negative stride or a strided innermost axis", st)
            _inside(ov, sum((n - 1) * s for n, s in zip(ov.shape[:-1], st[:-1])) + w, what)
            if what == "override":
                c.override_src[k] = ov.data_ptr()
                c.ov_s_net[k], c.ov_s_chain[k], c.ov_s_step[k], c.ov_s_job[k], c.ov_s_ent[k] = st[:5]
            else:
                c.override_base[k] = ov.data_ptr()
                c.ovb_s_net[k], c.ovb_s_chain[k], c.ovb_s_step[k], c.ovb_s_ent[k] = st[:4]


def policy_knockout_trace(actor_arena, critic_arena, which, spec, E, H, D, n_agents, jobs, hidden0_actor=None, hidden0_critic=None,
                          h_strides=(0, 0), avail=None, avail_strides=(0, 0), target=None, target_strides=(0, 0), n_actions=5, knock=None,
                          baseline=None, want=("kl",), packed=None, out=None, lib=None, override=None, override_base=None):
    """R_Actor (which=0) / R_Critic (1) / both (2) of every agent walked over the H consecutive steps of E recorded chains once per job,
    every job with its own GRU state from the common ``hidden0_*`` (iplan_ac_knockout_trace; include/iplan_hip.h:
    IplanAcKnockoutTraceArgs), forward only.  In steps 0 .. D-1 the job's entity has its columns of the knocked sources replaced as the
    features are gathered; steps D .. H-1 see the recorded rows.  ``spec`` (T = H), hidden0_*, avail, ``packed`` and their strides as for
    ``policy_trace``; ``jobs``, ``knock`` and ``baseline`` as for ``policy_knockout``.  ``target``: int64 a* by physical row with
    (s_net, s_row) strides, None (or an entry outside [0, n_actions)): the base chain's argmax of the step.  With D < H the rows' base gi
    comes from ``iplan_ac_trace`` with phases = 1, launched here first.  ``want``: "base" (probs [nA,E,H,n_actions], greedy, logp, values,
    target_action [nA,E,H] of the chain with nothing knocked) and, [nA,E,H,J] each, kl, dlogp, dvalue, greedy_ko (int64), logp_ko,
    values_ko, probs_ko [.., n_actions], "shift_sq" (shift_sq_actor / shift_sq_critic: the squared L2 distance of the job's state from the
    base chain's after the step), "h_ko" (h_ko_actor / h_ko_critic [.., 64]), "logp_all_ko" ([.., n_actions], the operands of kl; tests) and "gi_ko" (the knocked workspace [2, nA, E, D, ceil(J/15),
    16, 192] as a result; tests); those the selected nets do not provide are left out.  ``out``: optional dict of contiguous destinations.
    ``override`` / ``override_base``: per source, in the order of ``spec.sources``, views [nA, E, H, J, N, w] / [nA, E, H, N, w] or
    None -- ``policy_knockout``'s rules (any non-negative strides, innermost axis contiguous, read in place).  Job q reads an overridden
    source from its own view at EVERY step, not knocked as well; the base chain (and a job -1 without a view of its own) reads
    ``override_base`` where given, the batch otherwise.  With an override there is no ``iplan_ac_trace`` launch: one
    ``iplan_ac_knockout_chain`` launch runs the knocked trunk over all H steps (gi_ko is [2, nA, E, H, ceil(J/15), 16, 192]) and the same
    walk.  A base override needs a per-job override.
    Everything the kernels will read is bounds-checked here, on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    want = tuple(want)
    assert want and all(k in POLICY_KNOCKOUT_TRACE_OUTPUTS for k in want), want
    M = L.AC_HIDDEN
    assert 1 <= D <= H, (D, H)
    n_src = len(spec.sources)
    override, override_base = _per_source(override, n_src, "override"), _per_source(override_base, n_src, "override_base")
    chained = any(ov is not None for ov in override)
    assert chained or all(ov is None for ov in override_base), "a base override without a per-job override"
    c = L.AcKnockoutChainArgs() if chained else None
    a = c.kt if chained else L.AcKnockoutTraceArgs()
    b = a.base
    dev, last_row = _ac_rows(b, actor_arena, critic_arena, which, spec, E, H, n_agents)
    nets = n_agents * (2 if which == 2 else 1)
    stream = L.current_stream(dev)
    keep = [spec, hidden0_actor, hidden0_critic, avail, target, packed]
    keep += _job_list(a, jobs, spec.N, dev)
    J = a.J
    JT = (J + POLICY_KNOCKOUT_JOBS_PER_TILE - 1) // POLICY_KNOCKOUT_JOBS_PER_TILE
    if D < H and not chained:
        # the rows' base gi, once per row: the plain trunk over all E x H rows (the D knocked rows' entries are not read)
        ta, _, tkeep = policy_trace_args(actor_arena, critic_arena, which, spec, E, H, n_agents, n_actions=n_actions, want=(), packed=packed)
        ta.phases = 1
        _launch("ac_trace", lambda: lib.call("iplan_ac_trace", ta, stream), work=2.0 * nets * E * H * M * (spec.F + 5 * M))
        b.gi = ta.gi
        keep.append(tkeep)
    res = {}

    def dest(k, shape, dtype=torch.float32):
        return _dest(out, res, k, shape, dtype, dev)

    _chain_operands(b, which, n_agents, E, last_row, dev, n_actions, hidden0_actor, hidden0_critic, h_strides, avail, avail_strides, target,
                    target_strides, what="target")
    a.D = D
    assert (knock is None or len(knock) == n_src) and (baseline is None or len(baseline) == n_src), (knock, baseline, n_src)
    keep += _knock_baseline(a, spec, knock, baseline, dev)
    pair = (n_agents, E, H, J)
    _pair_dests(a, which, want, dest, pair, n_actions)
    if which != 1:
        _fill_acnet(b.actor, actor_arena, L.ACTOR_PARAM_ORDER, n_actions)
        if "base" in want:
            b.probs = dest("probs", (n_agents, E, H, n_actions))
            b.greedy = dest("greedy", (n_agents, E, H), torch.int64)
            b.logp = dest("logp", (n_agents, E, H))
            a.target_out = dest("target_action", (n_agents, E, H), torch.int64)
        if "logp_all_ko" in want:
            a.logp_all_ko = dest("logp_all_ko", pair + (n_actions,))
    if which != 0:
        _fill_acnet(b.critic, critic_arena, L.CRITIC_PARAM_ORDER, 1)
        if "base" in want:
            b.values = dest("values", (n_agents, E, H))
    for net, key in ((0, "actor"), (1, "critic")):
        if which == 1 - net:
            continue
        if "shift_sq" in want:
            setattr(a, "shift_sq_" + key, dest("shift_sq_" + key, pair))
        if "h_ko" in want:
            setattr(a, "h_ko_" + key, dest("h_ko_" + key, pair + (M,)))
    assert res, ("nothing of", want, "is provided by the selected nets")
    _ac_packed(b, which, packed)
    Dg = H if chained else D                                                  # the steps with knocked tiles of their own
    gi_shape = (2, n_agents, E, Dg, JT, 16, L.AC_TRACE_GI)
    if "gi_ko" in want:
        a.gi_ko = dest("gi_ko", gi_shape)
    else:
        gi_ko = workspace(dev, 2 * n_agents * E * Dg * JT * 16 * L.AC_TRACE_GI, "ac_knockout_trace")
        a.gi_ko = gi_ko.data_ptr()
        keep.append(gi_ko)
    work = 2.0 * nets * E * JT * 16 * M * (Dg * (spec.F + 5 * M) + H * 4 * M)
    if chained:
        _chain_overrides(c, spec, n_agents, E, H, J, dev, override, override_base)
        keep += [override, override_base]
        _launch("ac_knockout_chain", lambda: lib.call("iplan_ac_knockout_chain", c, stream), work=work)
    else:
        _launch("ac_knockout_trace", lambda: lib.call("iplan_ac_knockout_trace", a, stream), work=work)
    return res


def saliency_lag(actor_arena, critic_arena, which, spec, E, S, n_agents, lags, h_actor=None, h_critic=None, h_strides=(0, 0, 0), avail=None,
                 avail_strides=(0, 0, 0), target=None, target_strides=(0, 0, 0), target_all=-1, n_actions=5, want=("y", "entity"), packed=None,
                 out=None, lib=None):
    """Input gradients THROUGH TIME of R_Actor (which=0) / R_Critic (1) / both (2) of every agent on the slots (e, s) of E chains x S
    consecutive steps (iplan_ac_saliency_lag; include/iplan_hip.h: IplanAcSaliencyLagArgs): d y_s / d x_{s-k} for k = 0 .. ``lags``, in
    ``lags + 1`` launches, lag k seeded with the carry d y_s / d h_{s-k} lag k - 1 left.  Arguments as for ``saliency``, except that
    h_actor / h_critic hold the state ENTERING each step of a self-consistent chain (the caller's, from ``policy_trace``).  Results as
    ``saliency``'s with a lag axis behind the step axis of entity_* [nA,E,S,lags+1,N,n_src,2] and input_grad_* [nA,E,S,lags+1,F], and
    carry_actor / carry_critic [nA,E,S,lags+1,64], the carry after every lag; entries with s < k are NOT written (``out`` decides what
    they hold; fresh buffers are zeroed).  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    launches, res, _keep = saliency_lag_args(actor_arena, critic_arena, which, spec, E, S, n_agents, lags, h_actor, h_critic, h_strides, avail,
                                             avail_strides, target, target_strides, target_all, n_actions, want, packed, out)
    dev = (actor_arena if which != 1 else critic_arena).data.device
    nets = n_agents * (2 if which == 2 else 1)
    for a in launches:
        _launch("ac_saliency_lag", lambda: lib.call("iplan_ac_saliency_lag", a, L.current_stream(dev)),
                work=2.0 * nets * E * (S - a.lag) * L.AC_HIDDEN * (3 * spec.F + 17 * L.AC_HIDDEN))
    return res


def saliency_lag_args(actor_arena, critic_arena, which, spec, E, S, n_agents, lags, h_actor=None, h_critic=None, h_strides=(0, 0, 0), avail=None,
                      avail_strides=(0, 0, 0), target=None, target_strides=(0, 0, 0), target_all=-1, n_actions=5, want=("y", "entity"),
                      packed=None, out=None):
    """The descriptors of a ``saliency_lag`` call, one per lag in launch order, its output tensors and the operands to keep alive until
    the launches have been queued, checked but not launched: ([IplanAcSaliencyLagArgs], dict, tuple)."""
    assert isinstance(lags, int) and 0 <= lags < S, (lags, S)
    K1 = lags + 1
    M = L.AC_HIDDEN
    dev = (actor_arena if which != 1 else critic_arena).data.device
    n_src = sum(1 for s in spec.sources if s[1] > 0)
    nets = [k for k, on in (("actor", which != 1), ("critic", which != 0)) if on]
    shapes = {}
    for key in nets:
        shapes["carry_" + key] = (n_agents, E, S, K1, M)
        if "entity" in want:
            shapes["entity_" + key] = (n_agents, E, S, K1, spec.N, n_src, 2)
        if "input_grad" in want:
            shapes["input_grad_" + key] = (n_agents, E, S, K1, spec.F)
    lagged = {}
    for k, shape in shapes.items():
        _dest(out, lagged, k, shape, torch.float32, dev, fresh=torch.zeros)
    # the row description, the checks and the lag-0-only outputs are saliency's; the lagged outputs are set below
    base, res, keep = saliency_args(actor_arena, critic_arena, which, spec, E, S, n_agents, h_actor, h_critic, h_strides, avail, avail_strides,
                                    target, target_strides, target_all, n_actions, tuple(k for k in want if k in ("y", "act")) or ("y",), packed,
                                    out)
    if "y" not in want:
        for k in ("logp", "values", "target_action"):
            res.pop(k, None)
        base.logp = base.values = base.target_out = None
    res.update(lagged)
    launches = []
    for lag in range(K1):
        x = L.AcSaliencyLagArgs()
        C.memmove(C.byref(x.base), C.byref(base), C.sizeof(base))
        x.lag, x.n_lags = lag, K1
        x.seed_s_row = x.carry_s_row = K1 * M
        for key in nets:
            for k in ("entity_", "input_grad_"):
                if k + key in lagged:
                    setattr(x.base, k + key, lagged[k + key].data_ptr())
            carry = lagged["carry_" + key]
            setattr(x, "carry_" + key, carry.data_ptr() + 4 * M * lag)
            if lag:
                setattr(x, "seed_" + key, carry.data_ptr() + 4 * M * (lag - 1))
        launches.append(x)
    return launches, res, keep + (lagged,)


def ppo_eval(logp, entropy, values, old_logp, adv, value_preds, returns, mask, T, rows=None, clip=0.2, huber_delta=10.0,
             value_loss_coef=1.0, flags=0, n_parts=0, want=(), out=None, lib=None):
    """The PPO statistics of recorded rows under the nets, forward only (iplan_ppo_eval; include/iplan_hip.h: IplanPpoEvalArgs).
    logp / entropy / values [nA, rows]; old_logp / adv (RAW, normalised in the kernel over all row_stride entries) / value_preds /
    returns / mask [nA, row_stride], row r = b * T + t; ``rows`` defaults to logp's.  ``want``: which of the per-row outputs "ratio"
    [nA, rows] and "adv_norm" [nA, row_stride] to produce; ``out``: optional dict of contiguous destinations.  ``n_parts``:
    workgroups per agent -- any value gives the same bits.  Returns a dict: stats [nA, 16] (_lib.PPO_EVAL_STATS), step_stats
    [nA, T, 6] (_lib.PPO_EVAL_STEP_STATS) and the wanted per-row tensors."""
    lib = _lib(lib)
    a, res, _keep = ppo_eval_args(logp, entropy, values, old_logp, adv, value_preds, returns, mask, T, rows, clip, huber_delta,
                                  value_loss_coef, flags, n_parts, want, out, lib)
    _launch("ppo_eval", lambda: lib.call("iplan_ppo_eval", a, L.current_stream(logp.device)))
    return res


def ppo_eval_args(logp, entropy, values, old_logp, adv, value_preds, returns, mask, T, rows=None, clip=0.2, huber_delta=10.0,
                  value_loss_coef=1.0, flags=0, n_parts=0, want=(), out=None, lib=None):
    """The descriptor of a ``ppo_eval`` launch, its output tensors and the operands to keep alive until the launch has been
    queued, checked but not launched: (IplanPpoEvalArgs, dict, tuple)."""
    lib = _lib(lib)
    want = tuple(want)
    assert all(k in ("ratio", "adv_norm") for k in want), want
    dev = logp.device
    nA = logp.shape[0]
    rows = logp.shape[1] if rows is None else rows
    stride = old_logp.shape[1]
    for name, t, width in (("logp", logp, rows), ("entropy", entropy, rows), ("values", values, rows), ("old_logp", old_logp, stride),
                           ("adv", adv, stride), ("value_preds", value_preds, stride), ("returns", returns, stride), ("mask", mask, stride)):
        assert t.dtype == torch.float32 and t.device == dev and t.shape == (nA, width) and t.is_contiguous(), (name, t.shape, t.dtype, width)
    a = L.PpoEvalArgs()
    a.n_agents, a.rows, a.row_stride, a.T, a.n_parts = nA, rows, stride, T, n_parts
    a.logp, a.entropy, a.values, a.old_logp = logp.data_ptr(), entropy.data_ptr(), values.data_ptr(), old_logp.data_ptr()
    a.adv, a.value_preds, a.returns, a.mask = adv.data_ptr(), value_preds.data_ptr(), returns.data_ptr(), mask.data_ptr()
    a.clip, a.huber_delta, a.value_loss_coef, a.flags = clip, huber_delta, value_loss_coef, flags
    res = {}

    def dest(k, shape):
        return _dest(out, res, k, shape, torch.float32, dev)

    a.stats = dest("stats", (nA, len(L.PPO_EVAL_STATS)))
    a.step_stats = dest("step_stats", (nA, max(T, 0), len(L.PPO_EVAL_STEP_STATS)))
    if "ratio" in want:
        a.ratio = dest("ratio", (nA, rows))
    if "adv_norm" in want:
        a.adv_norm = dest("adv_norm", (nA, stride))
    ws = workspace(dev, max(int(lib.c.iplan_ppo_eval_workspace_bytes(nA, stride)), 8) // 4, "ppo_eval")
    a.workspace = ws.data_ptr()
    return a, res, (logp, entropy, values, old_logp, adv, value_preds, returns, mask, ws)


def ac_xhat_pack(spec, rows, n_agents, ln_stats, lib=None):
    """The normalised feature rows of a PPO batch, gathered once per train() into the two fragment-major copies the
    split-bf16 fc1 kernels stream (include/iplan_hip.h: IplanAcXhatArgs).  ``ln_stats``: the (mean, rstd) table a
    ``ac_forward(..., ln_stats_mode=1)`` pass stored for the same physical rows."""
    lib = _lib(lib)
    dev = ln_stats.device
    a = L.AcXhatArgs()
    a.n_agents, a.rows = n_agents, rows
    spec.fill(a.feat)
    assert ln_stats.dtype == torch.float32 and ln_stats.shape[0] == n_agents and ln_stats.stride(2) == 1 and ln_stats.stride(1) == 2
    a.ln_stats, a.ln_stats_s_net = ln_stats.data_ptr(), ln_stats.stride(0)
    nf, nb = (int(lib.c.iplan_ac_xhat_floats(C.byref(a.feat), rows, k)) for k in (0, 1))
    xf = torch.empty(n_agents, nf, dtype=torch.float32, device=dev)
    xb = torch.empty(n_agents, nb, dtype=torch.float32, device=dev)
    a.xf, a.xb = xf.data_ptr(), xb.data_ptr()
    _launch("ac_xhat_pack", lambda: lib.call("iplan_ac_xhat_pack", a, L.current_stream(dev)))
    return dict(xf=xf, xb=xb, rows=rows, n_agents=n_agents, KT=int(lib.c.iplan_ac_kpad(C.byref(a.feat))) // 16, _keep=(spec, ln_stats))


class _Packed(tuple):
    """(actor buffer, critic buffer) of Fc1Pack.get; ``fold`` says whether the W gamma / W beta tail is current"""
    fold = False


class Fc1Pack:
    """fc1.weight + feature_norm.{weight, bias} of the actor and critic arenas in the forward kernels' own K order and MFMA
    fragment order (iplan_ac_pack_fc1).  ``get(spec)`` repacks only when an arena changed since the last pack or the feature
    layout differs.  What counts as "changed" (the staleness key):
      * ``arena.version`` -- bumped by every kernel-side write (FusedAdam, DataParallel.broadcast_arena), by the modules'
        ``load_state_dict`` hook and by ``arena.touch()``;
      * the sum of ``p._version`` over the packed Parameters of all nets -- in-place writes THROUGH a Parameter (``p.add_()``,
        ``p.copy_()``, ``nn.init.*`` under no_grad, a torch.optim optimiser on ``mac.parameters()``) bump it.  The Parameters are
        bound to the arena with ``p.data = view``, which does NOT share the arena tensor's version counter, so
        ``arena.data._version`` says nothing about them;
      * ``arena.data._version`` -- writes on the arena tensor itself.
    A write through a detached alias (``p.data.mul_()``, a raw pointer) is invisible to all three: call ``arena.touch()``.
    ``fold=True`` also brings W gamma / W beta up to date (the rollout's folded LayerNorm(F) reads them; the streaming
    forward of a PPO epoch does not, and a repack after each of its 30 Adam steps would spend more on them than on the
    fragments)."""

    def __init__(self, actor_arena, critic_arena):
        self.arenas = (actor_arena, critic_arena)
        names = ("base.mlp.fc1.0.weight", "base.feature_norm.weight", "base.feature_norm.bias")
        self.watched = [[dict(m.named_parameters())[n] for m in arena.modules for n in names] for arena in self.arenas]
        self.buf = [None, None]
        self.key = [[None, None], [None, None]]             # per arena: key of the fragment part, of the W gamma / W beta part

    def get(self, spec, fold=False, lib=None):
        if os.environ.get("IPLAN_NO_FC1_PACK"):             # A/B knob: read the arena in place (scattered fragment loads)
            return None
        lib = _lib(lib)
        a = L.AcPackArgs()
        spec.fill(a.feat)
        floats = int(lib.c.iplan_ac_packed_floats(C.byref(a.feat)))
        sig = (spec.N, tuple(s[1] for s in spec.sources), spec.n_actions, spec.n_id)
        for k, (arena, order) in enumerate(zip(self.arenas, (L.ACTOR_PARAM_ORDER, L.CRITIC_PARAM_ORDER))):
            key = (arena.data._version, arena.version, sum(p._version for p in self.watched[k]), sig)
            if self.buf[k] is None or self.buf[k].shape[1] != floats:
                self.buf[k] = torch.empty(arena.n_nets, floats, dtype=torch.float32, device=arena.data.device)
                self.key[k] = [None, None]
            todo = [p for p, need in ((0, True), (1, fold)) if need and self.key[k][p] != key]
            if not todo:
                continue
            a.n_nets = arena.n_nets
            a.params, a.params_s_net = arena.data.data_ptr(), arena.net_stride
            a.off_w1, a.off_fn_w, a.off_fn_b = (arena.off(n) for n in ("base.mlp.fc1.0.weight", "base.feature_norm.weight", "base.feature_norm.bias"))
            a.packed, a.packed_s_net = self.buf[k].data_ptr(), floats
            a.parts = 0 if len(todo) == 2 else todo[0] + 1
            lib.call("iplan_ac_pack_fc1", a, L.current_stream(arena.data.device))
            for p in todo:
                self.key[k][p] = key
        out = _Packed((self.buf[0], self.buf[1]))
        out.fold = all(self.key[k][1] == self.key[k][0] for k in range(2))
        return out


# ---- weight gradients ----------------------------------------------------------------------------------
_WORKSPACES = {}
_SIDE_STREAMS = {}

def _side_stream(dev, *key):
    """one side stream per (device, caller's stream, tag), created on first use (dict.setdefault would construct -- and
    discard -- a stream per call and walk torch's 32-entry stream pool into aliasing streams already held)"""
    k = (str(dev),) + key
    s = _SIDE_STREAMS.get(k)
    if s is None:
        # side streams exist to run BESIDE the caller's stream: not on its hardware queue, and the encoder's BPTT stream (tag 2) not on
        # the forward / in-line stream's either (streams.distinct_stream: probed once, at creation)
        from .streams import distinct_stream, probe_mode
        avoid = [torch.cuda.current_stream(dev)]
        if probe_mode() == "full" and len(key) > 1 and key[1] == 2:
            avoid.append(_SIDE_STREAMS.get((str(dev), key[0])))
        s = _SIDE_STREAMS[k] = distinct_stream(dev, avoid)
    return s

_QUEUES_VERIFIED = set()


def verify_side_queues(dev, main, extra=None):
    """IPLAN_QUEUE_PROBE=verify (streams.probe_mode), once per (device, main stream), AFTER the side streams had their first use: the
    encoder's forward / BPTT side streams of ``main`` -- and the caller's ``extra`` roles {name: stream} (harness: the prediction
    learner's) -- must not share ``main``'s hardware queue nor each other's (the encoder's two may: they never run at the same time);
    one that does is replaced.  -> (list of replaced role names, {name: stream now in use})."""
    from .streams import distinct_stream, probe_mode, shares_queue
    key = (str(dev), main.cuda_stream)
    roles = dict(extra or {})
    k_f, k_b = (str(dev), main.cuda_stream), (str(dev), main.cuda_stream, 2)
    roles.update(enc_fwd=_SIDE_STREAMS.get(k_f), enc_bwd=_SIDE_STREAMS.get(k_b))
    if key in _QUEUES_VERIFIED and not extra:
        return [], roles
    _QUEUES_VERIFIED.add(key)
    if probe_mode() != "verify" or torch.device(dev).type != "cuda" or not hasattr(torch.cuda, "_sleep"):
        return [], roles
    replaced = []
    apart = lambda a, b: {a, b} != {"enc_fwd", "enc_bwd"}    # noqa: E731
    try:
        torch.cuda.synchronize(dev)
        for name in ["enc_bwd", "enc_fwd"] + [n for n in roles if n not in ("enc_bwd", "enc_fwd")]:
            s = roles.get(name)
            if s is None:
                continue
            keep_off = [main] + [o for n, o in roles.items() if n != name and o is not None and apart(name, n)]
            if any(shares_queue(o, s, dev) for o in keep_off):
                roles[name] = distinct_stream(dev, keep_off, force=True)
                replaced.append(name)
                if name == "enc_fwd":
                    _SIDE_STREAMS[k_f] = roles[name]
                elif name == "enc_bwd":
                    _SIDE_STREAMS[k_b] = roles[name]
        torch.cuda.synchronize(dev)
    except Exception as e:                                   # noqa: BLE001 -- never let the check cost the run
        import sys
        print(f"[iplan_amd] hardware-queue check skipped ({type(e).__name__}: {str(e)[:100]})", file=sys.stderr)
    return replaced, roles


_KSPLIT_BUFS = {}


class KernelTimers:
    """In-situ kernel timing for bench.py's roofline: HIP events recorded on the launch stream right around selected
    launches (every ``every[name]``-th one) while the real workload runs.  ``ops.TIMERS = KernelTimers(...)`` turns
    it on; ``summary()`` (after a device synchronise) gives {name: (launches timed, mean seconds, mean work)} where
    ``work`` is whatever the call site passed (algorithmic bytes / FLOPs of that launch; 0 if it passed nothing)."""

    def __init__(self, every=None):
        self.every = dict(every or {})
        self.count = {}
        self.spans = {}
        self.clocks = {}                                    # name -> device buffers of in-kernel stamps (read after a synchronise)

    def sample(self, name, every):
        n = self.count.get(name, 0)
        self.count[name] = n + 1
        return n % every == 0

    def launch(self, name, fn, stream=None, work=0.0):
        n = self.count.get(name, 0)
        self.count[name] = n + 1
        if n % self.every.get(name, 1):
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        self.spans.setdefault(name, []).append((e0, e1, float(work)))

    def summary(self):
        return {k: (len(v), sum(a.elapsed_time(b) for a, b, _ in v) / len(v) / 1e3, sum(w for _, _, w in v) / len(v))
                for k, v in self.spans.items()}


TIMERS = None


def _launch(name, fn, stream=None, work=0.0):
    """``stream``: the torch stream the launch goes to when it is not the current one (events must sit on that stream)."""
    if TIMERS is None:
        return fn()
    return TIMERS.launch(name, fn, stream, work)


def workspace(device, floats, tag="wgrad"):
    """Grow-only scratch buffer per (device, current stream, tag) -- owned by torch's caching allocator.  Keyed by
    stream because independent learners may run concurrently on different HIP streams."""
    sid = torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0
    key = (str(device), sid, tag)
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < floats:
        buf = torch.empty(max(int(floats), 1), dtype=torch.float32, device=device)
        _WORKSPACES[key] = buf
    return buf


class Wgrad:
    """Batch of dW = dY^T X problems (include/iplan_hip.h: IplanWgradProblem) written into a gradient arena."""

    def __init__(self, grad, n_nets, tag="iplan_wgrad"):
        self.grad, self.n_nets = grad, n_nets
        self.problems = []
        self._keep = []
        self.tag = tag                                      # KernelTimers key of the launches (bench.py's roofline entries)

    def add(self, dy, dy_strides, O, n_outer, n_inner, x=None, x_strides=(0, 0, 0), K=0, dw_off=-1, db_off=-1,
            dw_ld=None, dw_col0=0, seg=None, x_col0=0, x_shift=0, x0=None, x0_strides=(0, 0), beta=0.0, scale=1.0,
            dy_cg_stride=0, x_cg_stride=0, x_pre_valid=False):
        p = L.WgradProblem()
        p.dy = dy.data_ptr() if torch.is_tensor(dy) else dy
        p.dy_s_net, p.dy_s_outer, p.dy_s_inner = dy_strides
        if x is not None:
            p.x = x.data_ptr() if torch.is_tensor(x) else x
            p.x_s_net, p.x_s_outer, p.x_s_inner = x_strides
        if x0 is not None:
            p.x0 = x0.data_ptr() if torch.is_tensor(x0) else x0
            p.x0_s_net, p.x0_s_outer = x0_strides
        p.dw_off, p.db_off = dw_off, db_off
        p.O, p.K = O, K
        p.seg_split, p.seg_c0, p.seg_c1 = seg if seg is not None else (O, 0, 0)
        p.x_col0, p.x_shift, p.n_outer, p.n_inner = x_col0, x_shift, n_outer, n_inner
        p.dw_ld = K if dw_ld is None else dw_ld
        p.dw_col0 = dw_col0
        p.beta, p.scale = beta, scale
        p.dy_cg_stride, p.x_cg_stride, p.x_pre_valid = dy_cg_stride, x_cg_stride, int(bool(x_pre_valid))
        self.problems.append(p)
        self._keep += [dy, x, x0]
        return self

    def run(self, lib=None):
        lib = _lib(lib)
        dev = self.grad.device
        stream = L.current_stream(dev)
        for i0 in range(0, len(self.problems), L.WGRAD_MAX):
            chunk = self.problems[i0:i0 + L.WGRAD_MAX]
            a = L.WgradArgs()
            a.n_problems, a.n_nets = len(chunk), self.n_nets
            a.grad = self.grad.data_ptr()
            a.grad_s_net = self.grad.stride(0)
            for i, p in enumerate(chunk):
                a.p[i] = p
            need = lib.c.iplan_wgrad_workspace_floats(C.byref(a))
            ws = workspace(dev, need)
            a.workspace, a.workspace_floats = ws.data_ptr(), ws.numel()
            # algorithmic HBM bytes: every operand row of every problem read exactly once (4 (O + K) bytes per row) -- with the dY columns
            # two problems SHARE counted once (the two weights of a GRU: [dr dz] of the same rows; wgrad.hip pairs those jobs and does
            # read them once since round 5, so the figure is the least any kernel could move, not the least THIS kernel moves)
            nbytes = 4.0 * self.n_nets * sum(p.n_outer * p.n_inner * (p.O + p.K) for p in chunk)
            seen = {}
            for p in chunk:
                if p.O == 192 and p.K == 64 and p.seg_split >= 128:
                    key = (p.dy, p.dy_s_outer, p.dy_s_inner, p.n_outer, p.n_inner, p.seg_c0)
                    if key in seen:
                        nbytes -= 4.0 * self.n_nets * p.n_outer * p.n_inner * 128
                        del seen[key]
                    else:
                        seen[key] = True
            _launch(self.tag, lambda: lib.call("iplan_wgrad", a, stream), work=nbytes)


def _ac_wgrad(w, arena, head_names, saved, dsave, which, n_agents, rows, T, h, h_strides, T_phys, n_out, tiles, ln_part):
    """Weight-gradient problems of the 64-wide layers of one arena (actor or critic)."""
    M, SF, DS = L.AC_HIDDEN, L.AC_SAVE_FLOATS, L.AC_DSAVE_FLOATS
    sv = saved[which]                     # [n_agents, rows, SF]
    ds = dsave[which]                     # [n_agents, rows, DS]
    dptr, sptr = ds.data_ptr(), sv.data_ptr()
    dst = (rows * DS, DS, DS)
    sst = (rows * SF, SF, SF)
    off = arena.off
    # head: dY = dhead, X = f3 (slot 9)
    w.add(dptr + 4 * 6 * M, dst, n_out, rows, 1, x=sptr + 4 * 9 * M, x_strides=sst, K=M,
          dw_off=off(head_names[0]), db_off=off(head_names[1]))
    # GRU input weights: dgi = [dr, dz, dn_i] (cols 0..3M of the gate block), X = f2 (slot 3).  Rows indexed (episode, step) like the
    # hidden weights' problem below -- same dY pointer, strides and row split -- so that iplan_wgrad runs the two as ONE paired launch that
    # fetches [dr dz] once (wgrad.hip: wgrad_pair_bf16_kernel)
    n_ep = rows // T
    assert n_ep * T == rows
    w.add(dptr + 4 * 2 * M, (rows * DS, T * DS, DS), 3 * M, n_ep, T, x=sptr + 4 * 3 * M, x_strides=(rows * SF, T * SF, SF), K=M,
          dw_off=off("rnn.rnn.weight_ih_l0"), db_off=off("rnn.rnn.bias_ih_l0"))
    # GRU hidden weights: dgh = [dr, dz, dn_h], X = the stored hidden state of the row (episode layout)
    w.add(dptr + 4 * 2 * M, (rows * DS, T * DS, DS), 3 * M, n_ep, T, x=h, x_strides=(h_strides[0], T_phys * h_strides[1], h_strides[1]),
          K=M, dw_off=off("rnn.rnn.weight_hh_l0"), db_off=off("rnn.rnn.bias_hh_l0"), seg=(2 * M, 0, 3 * M))
    # fc2: dY = dz2, X = f1 (slot 1)
    w.add(dptr + 4 * M, dst, M, rows, 1, x=sptr + 4 * M, x_strides=sst, K=M,
          dw_off=off("base.mlp.fc2.0.0.weight"), db_off=off("base.mlp.fc2.0.0.bias"))
    # fc1 bias (S of the fc1 finalize)
    w.add(dptr, dst, M, rows, 1, db_off=off("base.mlp.fc1.0.bias"))
    # LayerNorm affine parameters: column sums of the per-tile partials
    lp = ln_part[which]                   # [n_agents, tiles, 6M]
    lst = (tiles * 6 * M, 6 * M, 6 * M)
    for k, name in enumerate(("rnn.norm", "base.mlp.fc2.0.2", "base.mlp.fc1.2")):
        w.add(lp.data_ptr() + 4 * (2 * k) * M, lst, M, tiles, 1, db_off=off(name + ".weight"))
        w.add(lp.data_ptr() + 4 * (2 * k + 1) * M, lst, M, tiles, 1, db_off=off(name + ".bias"))
    w._keep += [sv, ds, lp]


def n_which_rows(which, n_agents, rows):
    """rows x agents x nets of an actor/critic launch (which = 2: both nets)"""
    return (2 if which == 2 else 1) * n_agents * rows


def ac_backward(fwd, actor_arena, critic_arena, g_logp=None, g_entropy=0.0, g_values=None, lib=None):
    """Backward of an ``ac_forward(..., mode=2, save=True)`` launch: fills the gradient arenas of the
    nets that took part.  g_logp / g_values [n_agents, rows]; g_entropy: per-row tensor or a constant."""
    lib = _lib(lib)
    fa = fwd["_args"]
    which, n_agents, rows = fa.which, fa.n_agents, fa.rows
    spec, h_actor, h_critic = fwd["_keep"][0], fwd["_keep"][1], fwd["_keep"][2]
    saved = fwd["saved"]
    dev = saved.device
    f32 = dict(dtype=torch.float32, device=dev)
    a = L.AcBwdArgs()
    a.fwd = fa
    if which != 1:
        assert g_logp.shape == (n_agents, rows) and g_logp.is_contiguous()
        a.g_logp = g_logp.data_ptr()
        if torch.is_tensor(g_entropy):
            assert g_entropy.shape == (n_agents, rows) and g_entropy.is_contiguous()
            a.g_entropy = g_entropy.data_ptr()
        else:
            a.g_entropy_const = float(g_entropy)
        a.actor_grad = actor_arena.grad.data_ptr()
        a.actor_grad_s_net = actor_arena.grad.stride(0)
    if which != 0:
        assert g_values.shape == (n_agents, rows) and g_values.is_contiguous()
        a.g_values = g_values.data_ptr()
        a.critic_grad = critic_arena.grad.data_ptr()
        a.critic_grad_s_net = critic_arena.grad.stride(0)
    tiles = (rows + 15) // 16
    dsave = torch.empty(2, n_agents, rows, L.AC_DSAVE_FLOATS, **f32)
    ln_part = torch.empty(2, n_agents, tiles, L.AC_LNPART_FLOATS, **f32)
    a.dsave, a.ln_part = dsave.data_ptr(), ln_part.data_ptr()
    Fpad = int(lib.c.iplan_ac_kpad(C.byref(fa.feat)))
    n_which = 2 if which == 2 else 1
    xhat = fwd.get("_xhat")
    if xhat is not None:
        # split-bf16 form: a workgroup owns a block of k-tiles x both nets over a row chunk; the library sizes the chunks
        cr = C.c_int32(0)
        lib.c.iplan_ac_fc1_split_chunks(C.byref(fa.feat), n_agents, rows, C.byref(cr))
        chunk_rows = cr.value
        a.xb = xhat["xb"].data_ptr()
    else:
        # the fc1 contraction runs two waves per SIMD (8 k-tiles x 4 o-tiles per wave): as many row chunks as fill the chip once
        k_groups = int(lib.c.iplan_ac_fc1_groups(C.byref(fa.feat)))
        want = max(1, 2048 // (k_groups * n_which * n_agents))
        chunk_rows = max(256, ((rows + want - 1) // want + 15) // 16 * 16)
    chunks = (rows + chunk_rows - 1) // chunk_rows
    g_part = workspace(dev, n_which * n_agents * chunks * L.AC_HIDDEN * Fpad, "fc1")
    a.g_part, a.fc1_chunk_rows, a.fc1_chunks = g_part.data_ptr(), chunk_rows, chunks
    stream = L.current_stream(dev)
    # (algorithmic bytes: the record slots the tail reads -- a1, a2, the four gate rows, h', f3, the statistics -- + the row's hidden state,
    # the row gradients and the per-tile LayerNorm partials written)
    _launch("ac_bwd_tail_kernel", lambda: lib.call("iplan_ac_bwd_tail", a, stream),
            work=4.0 * n_which_rows(which, n_agents, rows) * (8 * L.AC_HIDDEN + 8 + L.AC_HIDDEN + L.AC_DSAVE_FLOATS + L.AC_LNPART_FLOATS / 16.0))
    ev_tail = None
    if which == 2 and dev.type == "cuda":
        ev_tail = torch.cuda.Event()
        ev_tail.record(torch.cuda.current_stream(dev))
    if xhat is not None:
        _launch("ac_fc1_split_wgrad", lambda: lib.call("iplan_ac_bwd_fc1_split", a, stream), work=2.0 * n_agents * rows * spec.F * 2 * L.AC_HIDDEN)
    else:
        lib.call("iplan_ac_bwd_fc1", a, stream)
    T, T_phys = spec.T, spec.T_phys
    hs = (fa.hs_net, fa.hs_row)
    # The weight-gradient contractions of the 64-wide layers are small, latency-bound launches (a wide one and three narrow
    # ones per arena, 0.25 ms per arena at config 3) and the two arenas are independent: the critic's run on a side stream
    # beside the actor's and the fc1 contraction, joined before the finalize (it reads both fc1.bias gradients).
    side = None
    if which == 2 and dev.type == "cuda" and not os.environ.get("IPLAN_AC_WGRAD_SERIAL"):
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev, main.cuda_stream, "ac")
        side.wait_event(ev_tail)
    if which != 1:
        w = Wgrad(actor_arena.grad, n_agents)
        _ac_wgrad(w, actor_arena, ("act.action_out.linear.weight", "act.action_out.linear.bias"), saved, dsave, 0,
                  n_agents, rows, T, h_actor.data_ptr(), hs, T_phys, fa.actor.n_out, tiles, ln_part)
        w.run(lib)
    if which != 0:
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            w = Wgrad(critic_arena.grad, n_agents)
            _ac_wgrad(w, critic_arena, ("v_out.weight", "v_out.bias"), saved, dsave, 1,
                      n_agents, rows, T, h_critic.data_ptr(), hs, T_phys, 1, tiles, ln_part)
            w.run(lib)
            if side is not None:
                ev_side = torch.cuda.Event()
                ev_side.record(side)
        if side is not None:
            main.wait_event(ev_side)
    lib.call("iplan_ac_bwd_fc1_finalize", a, stream)
    return dict(dsave=dsave, ln_part=ln_part)


def gat_backward(arena, saved, g_out, phase_clocks=None, lib=None):
    """Backward of a ``gat_forward(..., save=True)`` launch.  g_out [n_nets, B, N, A] (first two dims may
    be strided).  Fills arena.grad (every GAT parameter of every net)."""
    lib = _lib(lib)
    fa = saved["_args"]
    src0, src1, h_prev = saved["_keep"][0], saved["_keep"][1], saved["_keep"][2]
    n_nets, B, N, d0, d1 = fa.n_nets, fa.B, fa.N, fa.d0, fa.d1
    H = A = 32
    dev = g_out.device
    f32 = dict(dtype=torch.float32, device=dev)
    a = L.GatBwdArgs()
    a.fwd = fa
    a.g_out = g_out.data_ptr()
    a.g_s_net, a.g_s_b = _nb_strides(g_out, N * A)
    dgru = torch.empty(n_nets, 2, B, (N + 15) // 16, N - 1, 2, 3 * H, **f32)           # kernel-private scratch (class rows per tile and step)
    whh_part = torch.empty(n_nets, B, 2, 4, L.GAT_WHH_PART, **f32)
    a.whh_part, a.grad, a.grad_s_net = whh_part.data_ptr(), arena.grad.data_ptr(), arena.grad.stride(0)
    node_dy = torch.empty(n_nets, B * N, L.GAT_NODE_DY, **f32)
    hard_part = torch.empty(n_nets, B, L.GAT_HARD_PART, **f32)
    a.dgru, a.node_dy, a.hard_part = dgru.data_ptr(), node_dy.data_ptr(), hard_part.data_ptr()
    if phase_clocks is not None:                            # int64 [>= 15]: workgroup 0's clocks land in slots 8..14
        assert phase_clocks.dtype == torch.int64 and phase_clocks.numel() >= 15
        a.fwd.phase_clocks = phase_clocks.data_ptr()
    _launch("gat_bwd_kernel", lambda: lib.call("iplan_gat_bwd", a, L.current_stream(dev)))
    a.fwd.phase_clocks = fa.phase_clocks

    w = Wgrad(arena.grad, n_nets)
    off = arena.off
    DYW = L.GAT_NODE_DY
    nd = node_dy.data_ptr()
    nst = (B * N * DYW, N * DYW, DYW)                       # rows (b, i)
    D = d0 + d1
    # encoding: dY = ENC, X = [src0 || src1] rows
    w.add(nd, nst, H, B, N, x=src0, x_strides=(src0.stride(0), src0.stride(1), d0), K=d0,
          dw_off=off("encoding.weight"), dw_ld=D, db_off=off("encoding.bias"))
    if d1 > 0:
        w.add(nd, nst, H, B, N, x=src1, x_strides=(src1.stride(0), src1.stride(1), d1), K=d1,
              dw_off=off("encoding.weight"), dw_ld=D, dw_col0=d0)
    he = saved["h_enc"]
    hst = (B * N * H, N * H, H)
    gru = saved["gru"]
    P1 = N - 1
    for dr, sfx in ((0, ""), (1, "_reverse")):
        # separable input projection: W_ih = [W_a | W_b]
        w.add(nd + 4 * (32 + dr * 192), nst, 3 * H, B, N, x=he, x_strides=hst, K=H,
              dw_off=off("hard_bi_GRU.weight_ih_l0" + sfx), dw_ld=2 * H, db_off=off("hard_bi_GRU.bias_ih_l0" + sfx))
        w.add(nd + 4 * (128 + dr * 192), nst, 3 * H, B, N, x=he, x_strides=hst, K=H,
              dw_off=off("hard_bi_GRU.weight_ih_l0" + sfx), dw_ld=2 * H, dw_col0=H)
        # (recurrent weights hard_bi_GRU.weight_hh / bias_hh: accumulated by the backward kernel itself)
        # hard_encoding.weight[c][dr*H : (dr+1)*H] = -/+ sum dDelta * h  (per-scene partials from the kernel)
        for c, sc in ((0, -1.0), (1, 1.0)):
            w.add(hard_part.data_ptr() + 4 * dr * 4 * H, (B * L.GAT_HARD_PART, L.GAT_HARD_PART, H), H, B, 4,
                  db_off=off("hard_encoding.weight") + c * 2 * H + dr * H, scale=sc)
    for c, sc in ((0, -1.0), (1, 1.0)):
        w.add(hard_part.data_ptr() + 4 * 8 * H, (B * L.GAT_HARD_PART, L.GAT_HARD_PART, L.GAT_HARD_PART), 1, B, 1,
              db_off=off("hard_encoding.bias") + c, scale=sc)
    w.add(nd + 4 * 416, nst, A, B, N, x=he, x_strides=hst, K=H, dw_off=off("q.weight"))
    w.add(nd + 4 * 448, nst, A, B, N, x=he, x_strides=hst, K=H, dw_off=off("k.weight"))
    w.add(nd + 4 * 480, nst, A, B, N, x=he, x_strides=hst, K=H, dw_off=off("v.weight"), db_off=off("v.bias"))
    xs = saved["x"]
    w.add(nd + 4 * 512, nst, 3 * A, B, N, x=xs, x_strides=(B * N * A, N * A, A), K=A,
          dw_off=off("rnn.weight_ih"), db_off=off("rnn.bias_ih"))
    w.add(nd + 4 * 512, nst, 3 * A, B, N, x=h_prev, x_strides=(h_prev.stride(0), h_prev.stride(1), A), K=A,
          dw_off=off("rnn.weight_hh"), db_off=off("rnn.bias_hh"), seg=(2 * A, 0, 3 * A))
    w._keep += [dgru, node_dy, hard_part, saved]
    w.run(lib)
    return dict(dgru=dgru, node_dy=node_dy, hard_part=hard_part)


# ---- prediction decoder --------------------------------------------------------------------------------
def pdec_forward(arena, x0, h0, target, mask, N, keep=None, drop_p=0.0, teacher=None, mask_sum=None, lib=None):
    """Prediction_Decoder.forward + masked-L1 loss for all nets.  x0 [n_nets, rows, d], h0 [n_nets, rows, 32],
    target [n_nets, rows, P, d], mask [n_nets, rows // N], keep [n_nets, P, rows, 32] or None, teacher int32
    [n_nets, P] or None.  Returns dict(pred, loss [n_nets], saved, ...)."""
    lib = _lib(lib)
    n_nets, rows, d = x0.shape
    P = target.shape[2]
    dev = x0.device
    f32 = dict(dtype=torch.float32, device=dev)
    for t in (x0, h0, target, mask):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert h0.shape == (n_nets, rows, 32) and target.shape == (n_nets, rows, P, d) and mask.shape == (n_nets, rows // N)
    a = L.PdecArgs()
    a.n_nets, a.rows, a.N, a.P, a.d = n_nets, rows, N, P, d
    a.x0, a.h0, a.target, a.mask = x0.data_ptr(), h0.data_ptr(), target.data_ptr(), mask.data_ptr()
    if keep is not None:
        assert keep.shape == (n_nets, P, rows, 32) and keep.is_contiguous() and keep.dtype == torch.float32
        a.keep = keep.data_ptr()
    a.drop_p = drop_p
    if teacher is not None:
        assert teacher.dtype == torch.int32 and teacher.shape == (n_nets, P) and teacher.is_contiguous()
        a.teacher = teacher.data_ptr()
    a.params, a.params_s_net = arena.data.data_ptr(), arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.off[i] = arena.off(k)
    if mask_sum is not None:                               # loss normaliser over all data-parallel ranks' samples
        assert mask_sum.shape == (n_nets,) and mask_sum.dtype == torch.float32 and mask_sum.is_contiguous()
        a.mask_sum = mask_sum.data_ptr()
    tiles = (rows + 15) // 16
    out = dict(pred=torch.empty(n_nets, rows, P, d, **f32), saved=torch.empty(n_nets, rows, P, L.PDEC_SAVE, **f32),
               loss_part=torch.empty(n_nets, tiles, **f32), loss=torch.empty(n_nets, **f32))
    a.pred, a.saved, a.loss_part, a.loss = (out[k].data_ptr() for k in ("pred", "saved", "loss_part", "loss"))
    lib.call("iplan_pdec_fwd", a, L.current_stream(dev))
    out["_args"] = a
    out["_keep"] = (x0, h0, target, mask, keep, teacher)
    return out


def pdec_backward(arena, fwd, lib=None):
    """Backward of pdec_forward's loss (d loss = 1 per net): fills arena.grad, returns dLoss/dh0 [n_nets, rows, 32]."""
    lib = _lib(lib)
    a = fwd["_args"]
    n_nets, rows, P, d = a.n_nets, a.rows, a.P, a.d
    h0 = fwd["_keep"][1]
    dev = h0.device
    dsave = torch.empty(n_nets, rows, P, L.PDEC_DSAVE, dtype=torch.float32, device=dev)
    g_h0 = torch.empty(n_nets, rows, 32, dtype=torch.float32, device=dev)
    a.dsave, a.g_h0 = dsave.data_ptr(), g_h0.data_ptr()
    lib.call("iplan_pdec_bwd", a, L.current_stream(dev))
    SV, DS, H = L.PDEC_SAVE, L.PDEC_DSAVE, 32
    sv, dp = fwd["saved"].data_ptr(), dsave.data_ptr()
    sst, dst = (rows * P * SV, P * SV, SV), (rows * P * DS, P * DS, DS)
    off = arena.off
    w = Wgrad(arena.grad, n_nets)
    w.add(dp, dst, d, rows, P, x=sv + 4 * 208, x_strides=sst, K=H, dw_off=off("decoder.out.weight"), db_off=off("decoder.out.bias"))
    w.add(dp + 4 * 48, dst, 3 * H, rows, P, x=sv + 4 * 16, x_strides=sst, K=H,
          dw_off=off("decoder.rnn.weight_ih_l0"), db_off=off("decoder.rnn.bias_ih_l0"))
    w.add(dp + 4 * 48, dst, 3 * H, rows, P, x=sv + 4 * 176, x_strides=sst, K=H, x_shift=-1, x0=h0, x0_strides=(rows * H, H),
          dw_off=off("decoder.rnn.weight_hh_l0"), db_off=off("decoder.rnn.bias_hh_l0"), seg=(2 * H, 0, 3 * H))
    w.add(dp + 4 * 16, dst, H, rows, P, x=sv, x_strides=sst, K=d, dw_off=off("decoder.linear.weight"), db_off=off("decoder.linear.bias"))
    w._keep += [dsave, fwd]
    w.run(lib)
    return g_h0


def predict(arena, hist, offset, ent_stride, step_stride, h0, N, P, d, want_pred=True, want_metrics=False, target=None, weight=None,
            presence_col=-1, pos=(1, 2), checked=False, lib=None):
    """Prediction_Decoder.forward in eval mode (no teacher forcing, no dropout, nothing saved) for all nets, with the start
    state and the targets read in place.  ``hist``: any fp32 tensor whose storage holds the states (e.g. the episode buffer's
    history field); ``offset`` int64 [n_nets, S]: element offset, from hist's first element, of (sample, entity 0, feature 0);
    entity i's row is ``ent_stride`` elements further per entity, the target of horizon step p ``(p + 1) * step_stride``
    elements further, read from ``target`` (default: ``hist``; only with ``want_metrics``).  h0 [n_nets, S*N, 32] contiguous,
    ``weight`` [n_nets, S] or None (= 1), ``pos`` = the position columns (consecutive), ``presence_col`` < 0 = no presence factor.
    Unless ``checked`` (the caller has already done it on the host) the offsets are read back and checked against the storage.
    Returns dict(pred [n_nets, S*N, P, d] or None, metrics [n_nets, P, 3] or None: sums of w * ||d pos||, w * |d|_1, w)."""
    lib = _lib(lib)
    n_nets, S = offset.shape
    dev = h0.device
    f32 = dict(dtype=torch.float32, device=dev)
    assert want_pred or want_metrics
    assert offset.dtype == torch.int64 and offset.is_contiguous() and offset.device == dev
    assert hist.dtype == torch.float32 and hist.device == dev
    assert h0.shape == (n_nets, S * N, 32) and h0.is_contiguous() and h0.dtype == torch.float32
    assert 1 <= d <= 16 and P >= 1 and 1 <= n_nets <= L.MAX_NETS and ent_stride >= 0 and step_stride >= 0
    if want_metrics and target is None:
        target = hist
    if not want_metrics:
        target = None

    if not checked:
        lo, hi = int(offset.min()), int(offset.max())
        assert lo >= 0 and hi + (N - 1) * ent_stride + d <= _room(hist), ("start rows outside hist", lo, hi, _room(hist))
        if target is not None:
            assert target.dtype == torch.float32 and target.device == dev
            assert hi + (N - 1) * ent_stride + P * step_stride + d <= _room(target), ("target rows outside target", hi, _room(target))
    a = L.PredictArgs()
    a.n_nets, a.S, a.N, a.P, a.d = n_nets, S, N, P, d
    a.x0, a.offset, a.ent_stride, a.step_stride, a.h0 = hist.data_ptr(), offset.data_ptr(), ent_stride, step_stride, h0.data_ptr()
    a.presence_col, a.pos_first, a.pos_count = -1, 0, 1
    a.params, a.params_s_net = arena.data.data_ptr(), arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.off[i] = arena.off(k)
    out = dict(pred=None, metrics=None)
    if want_pred:
        out["pred"] = torch.empty(n_nets, S * N, P, d, **f32)
        a.pred = out["pred"].data_ptr()
    part = None
    if want_metrics:
        pos = tuple(int(c) for c in pos)
        assert len(pos) >= 1 and pos == tuple(range(pos[0], pos[0] + len(pos))) and 0 <= pos[0] and pos[-1] < d, pos
        assert presence_col < d
        a.target = target.data_ptr()
        a.presence_col, a.pos_first, a.pos_count = max(presence_col, -1), pos[0], len(pos)
        if weight is not None:
            assert weight.shape == (n_nets, S) and weight.dtype == torch.float32 and weight.is_contiguous() and weight.device == dev
            a.weight = weight.data_ptr()
        out["metrics"] = torch.empty(n_nets, P, 3, **f32)
        part = torch.empty(n_nets, P, 3, (S * N + 15) // 16, **f32)
        a.metrics, a.part = out["metrics"].data_ptr(), part.data_ptr()
    lib.call("iplan_predict", a, L.current_stream(dev))
    out["_args"] = a
    out["_keep"] = (hist, target, offset, h0, weight, part)
    return out


PREDICT_KNOCKOUT_OUTPUTS = ("fshift_sq", "ferr_sq", "pred_ko")


def predict_knockout(arena, history, latent_ko, start, P, pred_base=None, pos=(1, 2), want=("fshift_sq",), out=None, lib=None):
    """``predict``'s decoder chain run on the latents ``gat_knockout_trace`` wrote, reduced in the kernel to P numbers per row
    (iplan_predict_knockout), forward only.  history [n_nets,B,S,N,d]: the episode field, a view whose first four dims may be strided
    arbitrarily, read in place and never knocked -- row (net, b, start + h, i) is the chain's start state, rows start + h + 1 + p its
    targets.  latent_ko [n_nets,B,J,H,N,32] (first four dims strided, 16-byte aligned rows): the chains' h_0; the window is steps
    start .. start + H - 1.  ``pos``: up to 16 distinct columns in [0, d), added in the order given.  ``want``: which of fshift_sq
    [n_nets,B,J,H,N,P] (sum over pos of (pred_ko - pred_base)^2; needs ``pred_base`` [n_nets,B,H,N,P,d], first three dims strided:
    ``predict``'s forecasts on the walk with nothing knocked, written by an earlier launch), ferr_sq [n_nets,B,J,H,N,P] (the same sum
    against the recorded future, +0.0 where the target step start + h + 1 + p is not recorded) and pred_ko [n_nets,B,J,H,N,P,d] to
    produce; ``out``: optional dict of destination views for some of them (the same layouts, first four dims strided).  Everything
    the kernel will touch is bounds-checked here, on the host.  Returns a dict of the wanted tensors."""
    lib = _lib(lib)
    a, res, keep = predict_knockout_args(arena, history, latent_ko, start, P, pred_base, pos, want, out)
    _launch("predict_knockout_kernel", lambda: lib.call("iplan_predict_knockout", a, L.current_stream(history.device)))
    res["_args"] = a
    res["_keep"] = keep
    return res


def predict_knockout_args(arena, history, latent_ko, start, P, pred_base=None, pos=(1, 2), want=("fshift_sq",), out=None):
    """The descriptor of a ``predict_knockout`` launch, its output tensors and what must stay alive until the launch has been queued,
    checked but not launched: (IplanPredictKnockoutArgs, dict, list)."""
    n_nets, B, S, N, d = history.shape
    A = 32
    dev = history.device
    want = tuple(want)
    assert want and all(k in PREDICT_KNOCKOUT_OUTPUTS for k in want), want
    assert latent_ko.dim() == 6 and latent_ko.shape[:2] == (n_nets, B) and latent_ko.shape[4:] == (N, A) and latent_ko.device == dev, latent_ko.shape
    J, H = latent_ko.shape[2:4]
    start, P = int(start), int(P)
    assert 1 <= d <= 16 and P >= 1 and J >= 1 and H >= 1 and 1 <= n_nets <= L.MAX_NETS, (d, P, J, H, n_nets)
    assert 0 <= start and start + H <= S, (start, H, S)
    assert B * J * H * N <= 0x7fffffff - 16, (B, J, H, N)
    pos = tuple(int(c) for c in pos)
    assert 1 <= len(pos) <= 16 and len(set(pos)) == len(pos) and all(0 <= c < d for c in pos), (pos, d)
    a = L.PredictKnockoutArgs()
    a.n_nets, a.B, a.J, a.H, a.N, a.P, a.d, a.S, a.start = n_nets, B, J, H, N, P, d, S, start
    a.n_pos = len(pos)
    for k, c in enumerate(pos):
        a.pos[k] = c
    # the history view: (net, b, step, entity) strided, d contiguous floats per row, every recorded step inside the storage
    assert history.dtype == torch.float32 and (history.stride(4) == 1 or d == 1), history.stride()
    hs = history.stride()[:4]
    assert all(x >= 0 for x in hs), hs
    _inside(history, sum((history.shape[k] - 1) * hs[k] for k in range(4)) + d, "predict_knockout: history")
    a.history = history.data_ptr()
    a.hist_s_net, a.hist_s_b, a.hist_s_step, a.hist_s_ent = hs
    keep = [history, latent_ko, pred_base]
    probe = {}
    _, *ls = _dest_nbjs({"latent_ko": latent_ko}, probe, "latent_ko", (n_nets, B, J, H), (N, A), dev)
    assert latent_ko.data_ptr() % 16 == 0 and all(x % 4 == 0 for x in ls), ("latent_ko must be 16-byte aligned with strides % 4 == 0", ls)
    a.latent_ko = latent_ko.data_ptr()
    a.lat_s_net, a.lat_s_b, a.lat_s_job, a.lat_s_step = ls
    if pred_base is not None:
        assert pred_base.shape == (n_nets, B, H, N, P, d) and pred_base.device == dev, pred_base.shape
        a.pred_base = pred_base.data_ptr()
        a.pb_s_net, a.pb_s_b, a.pb_s_step = _nbs_strides(pred_base, N * P * d, "pred_base")
    assert "fshift_sq" not in want or pred_base is not None, "fshift_sq needs pred_base, the forecasts of the window with nothing knocked"
    a.params, a.params_s_net = arena.data.data_ptr(), arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.off[i] = arena.off(k)
    res = {}
    pre = {"fshift_sq": "fs", "ferr_sq": "fe", "pred_ko": "pk"}
    for k in want:
        inner = (N, P, d) if k == "pred_ko" else (N, P)
        t, *s = _dest_nbjs(out, res, k, (n_nets, B, J, H), inner, dev)
        setattr(a, k, t.data_ptr())
        for name, v in zip(("net", "b", "job", "step"), s):
            setattr(a, f"{pre[k]}_s_{name}", v)
    return a, res, keep


PDEC_SAL_OUTPUTS = ("state_grad", "latent_grad", "state_l1", "state_gxi", "latent_l1", "latent_gxi", "pred", "active")


def pdec_saliency(arena, hist, offset, ent_stride, h0, N, P, d, jobs, v=None, want=("state_l1", "latent_l1"), out=None, checked=False, lib=None):
    """d <v, y_p> / d x0 and / d h0 of the chain ``predict`` walks (csrc/pdec_saliency.hip), per row and job, for all nets.  ``hist``,
    ``offset`` int64 [n_nets, S], ``ent_stride``, ``h0`` [n_nets, S*N, 32]: as ``predict`` (the start state is read in place).  ``jobs``:
    K pairs (p, c) -- horizon step p in [0, P) and the output column c in [0, d) whose one-hot is the cotangent, or c = None / -1 for
    the row ``v[net, row, p, :]`` of ``v`` [n_nets, S*N, P, d] (contiguous).  ``want``: names out of PDEC_SAL_OUTPUTS.  Returns a dict
    with state_grad [n_nets, S*N, K, d], latent_grad [n_nets, S*N, K, 32], state_l1 / state_gxi / latent_l1 / latent_gxi [n_nets, S*N, K],
    pred [n_nets, S*N, P, d], active int32 [n_nets, S*N, P] (a 32-bit mask), None for what was not asked for.  ``out``: optional dict of
    destination tensors of exactly those shapes (contiguous) for some of the wanted names.  Unless ``checked`` the offsets are read
    back and checked against hist's storage."""
    lib = _lib(lib)
    n_nets, S = offset.shape
    dev = h0.device
    want = tuple(want)
    assert all(k in PDEC_SAL_OUTPUTS for k in want), want
    assert offset.dtype == torch.int64 and offset.is_contiguous() and offset.device == dev
    assert hist.dtype == torch.float32 and hist.device == dev
    assert h0.shape == (n_nets, S * N, 32) and h0.is_contiguous() and h0.dtype == torch.float32
    assert ent_stride >= 0
    if not checked:
        lo, hi = int(offset.min()), int(offset.max())
        assert lo >= 0, ("start rows outside hist", lo)
        _inside(hist, hi + (N - 1) * ent_stride + d, "pdec_saliency: hist")
    jobs = [(int(p), -1 if c is None else int(c)) for p, c in jobs]
    K, rows = len(jobs), S * N
    a = L.PdecSaliencyArgs()
    a.n_nets, a.S, a.N, a.P, a.d, a.K = n_nets, S, N, P, d, K
    a.x0, a.offset, a.ent_stride, a.h0 = hist.data_ptr(), offset.data_ptr(), ent_stride, h0.data_ptr()
    a.params, a.params_s_net = arena.data.data_ptr(), arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.off[i] = arena.off(k)
    flat = [x for job in jobs for x in job]
    j_host = (C.c_int32 * max(2 * K, 2))(*flat)
    j_dev = torch.tensor(flat, dtype=torch.int32, device=dev) if K else None
    a.jobs, a.jobs_host = L.ptr(j_dev), C.cast(j_host, C.c_void_p)
    if v is not None:
        assert v.dtype == torch.float32 and v.device == dev and v.is_contiguous() and v.shape == (n_nets, rows, P, d), v.shape
        a.v = v.data_ptr()
    shapes = dict(state_grad=(K, d), latent_grad=(K, 32), state_l1=(K,), state_gxi=(K,), latent_l1=(K,), latent_gxi=(K,), pred=(P, d), active=(P,))
    res = {k: None for k in PDEC_SAL_OUTPUTS}
    for k in want:
        shape = (n_nets, rows) + shapes[k]
        dt = torch.int32 if k == "active" else torch.float32
        if out is not None and k in out:
            t = out[k]
            assert t.shape == shape and t.dtype == dt and t.is_contiguous() and t.device == dev, (k, t.shape, shape)
        else:
            t = torch.empty(shape, dtype=dt, device=dev)
        res[k] = t
        setattr(a, k, t.data_ptr())
    _launch("pdec_sal_kernel", lambda: lib.call("iplan_pdec_saliency", a, L.current_stream(dev)))
    res["_args"] = a
    res["_keep"] = (hist, offset, h0, j_host, j_dev, v)
    return res


# ---- behaviour learning ---------------------------------------------------------------------------------
def _beh_pieces(which, default):
    """Window pieces of the behaviour forward / backward pipelines (IPLAN_BEH_PIECES[_FWD|_BWD]: tuning / test knobs)."""
    return int(os.environ.get("IPLAN_BEH_PIECES_" + which, os.environ.get("IPLAN_BEH_PIECES", str(default))))


def _piece_bounds(J, pieces):
    """Window ranges of the pipelined behaviour forward / BPTT: ``pieces`` equal ranges behind ONE short range at the low end
    (windows [0, J // 16)).  The forward walks the ranges bottom up and its decoder can only start once the encoder has
    finished the first range; the BPTT walks them top down and the encoder's BPTT of the last range -- plus the gradient
    reduction and the optimiser step the next rollout waits for -- trails the decoder's.  With equal ranges both waits were a
    whole range of encoder work (0.65 ms in front of the decoder forward, 1.3 ms behind the decoder BPTT: rocprofv3 trace of
    a training cycle, profiles/history/r02h_cycle_trace_learn_phase.txt); the short range makes them a sixteenth of the episode."""
    if pieces <= 1 or J < 4 * pieces or os.environ.get("IPLAN_BEH_EQUAL_PIECES"):
        return [round(J * k / pieces) for k in range(pieces + 1)]
    s0 = max(1, J // 16)
    return [0] + [s0 + round((J - s0) * k / pieces) for k in range(pieces + 1)]


def _beh_thin_in_kernel():
    """decoder BPTT second form with the thin weight gradients accumulated in the kernel (the default): not with the first form
    (IPLAN_DEC_BWD_V1=1) nor with the A/B knob IPLAN_DEC_THIN_ROWS=1"""
    return not os.environ.get("IPLAN_DEC_BWD_V1") and not os.environ.get("IPLAN_DEC_THIN_ROWS")


def beh_forward(enc_arena, dec_arena, hist, mask, L_win, Z, coef, thres, drop_p, keep=None, seed=0, hard=False, win_norm=None,
                lib=None):
    """Forward of Behavior_policy.learn for all nets.  hist [n_nets, E, T, N, d] (first three dims may be
    strided), mask [n_nets, E, T] contiguous, keep uint8 [n_nets, J, E*N, L, 64] or None (in-kernel draw from
    ``seed``).  Returns dict(loss [n_nets, 2] = (behaviour, stability), saved...)."""
    lib = _lib(lib)
    n_nets, E, T, N, d = hist.shape
    assert hist.dtype == torch.float32 and hist.stride(4) == 1 and hist.stride(3) == d
    assert mask.shape == (n_nets, E, T) and mask.is_contiguous() and mask.dtype == torch.float32
    dev = hist.device
    f32 = dict(dtype=torch.float32, device=dev)
    J = (T // L_win - 1) if hard else (T - 1 - L_win)
    rows = E * N
    a = L.BehArgs()
    a.n_nets, a.E, a.N, a.T, a.L, a.d, a.Z = n_nets, E, N, T, L_win, d, Z
    a.hard = 1 if hard else 0
    a.hist, a.h_s_net, a.h_s_e, a.h_s_t = hist.data_ptr(), hist.stride(0), hist.stride(1), hist.stride(2)
    a.mask = mask.data_ptr()
    if keep is not None:
        assert keep.dtype == torch.uint8 and keep.shape == (n_nets, J, rows, L_win, 64) and keep.is_contiguous()
        a.keep = keep.data_ptr()
    a.seed, a.drop_p, a.coef, a.thres = seed, drop_p, coef, thres
    # the output layer's input is only read by the out.weight contraction of iplan_wgrad; the BPTT's second form accumulates that
    # gradient itself (beh_backward: ``thin``) and the forward then need not store it (64 of 480 floats per chain-step)
    a.fwd_skip_act = 1 if (_beh_thin_in_kernel() and not os.environ.get("IPLAN_FWD_SAVE_ACT")) else 0     # (IPLAN_FWD_SAVE_ACT=1: A/B knob)
    if win_norm is not None:                               # per-window mask sums over all data-parallel ranks' envs
        assert win_norm.shape == (n_nets, J) and win_norm.dtype == torch.float32 and win_norm.is_contiguous()
        a.win_norm = win_norm.data_ptr()
    a.enc_params, a.enc_s_net = enc_arena.data.data_ptr(), enc_arena.net_stride
    for i, k in enumerate(L.ENC_PARAM_ORDER):
        a.enc_off[i] = enc_arena.off(k)
    a.dec_params, a.dec_s_net = dec_arena.data.data_ptr(), dec_arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.dec_off[i] = dec_arena.off(k)
    tiles = (rows + 15) // 16
    # decoder record, column-grouped: [net, chain tile, 16-column group (31), step (J * L), chain (16), 16] -- a wave's store of one
    # 16-column group of its 16 chains is ONE contiguous 1 KiB block (5.6 instead of 3.3 TB/s of stores, scripts/ubench/
    # record_store.hip), and a column group's rows are contiguous over (step, chain) for the weight-gradient contraction.  The chain
    # slots of a ragged last tile are never written by the kernels: zeroed here, they add nothing to the gradients.
    out = dict(saved_dec=torch.empty(n_nets, tiles, L.BEH_SAVE_DEC // 16, J * L_win, 16, 16, **f32),
               saved_enc=torch.empty(n_nets, tiles, L.BEH_SAVE_ENC // 16, J * L_win, 16, 16, **f32),     # column-grouped too
               saved_lat=torch.empty(n_nets, rows, J, L.BEH_SAVE_LAT, **f32),
               loss_part=torch.empty(n_nets, tiles, 2, **f32), loss=torch.empty(n_nets, 2, **f32))
    if rows % 16:
        out["saved_dec"][:, -1, :, :, rows % 16:].zero_()
    for k in ("saved_dec", "saved_enc", "saved_lat", "loss_part", "loss"):
        setattr(a, k, out[k].data_ptr())
    # Pipeline (GPU): the decoder holds 138 of the 256 CUs for the whole episode, so the forward runs in window pieces --
    # the encoder of piece k+1 on a side stream beside the decoder of piece k on the main stream.
    side = None
    if dev.type == "cuda" and not os.environ.get("IPLAN_BEH_SERIAL"):
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev, main.cuda_stream)
    pieces = max(1, min(_beh_pieces("FWD", 4 if side is not None else 1), J))
    stream = L.current_stream(dev)
    if pieces == 1:
        lib.call("iplan_beh_fwd", a, stream)
    else:
        bounds = _piece_bounds(J, pieces)
        pieces = len(bounds) - 1
        out["enc_carry"] = torch.empty(n_nets, tiles, 768, **f32)
        out["dec_carry"] = torch.empty(n_nets, tiles, 2, 512, **f32)
        a.enc_carry, a.dec_carry = out["enc_carry"].data_ptr(), out["dec_carry"].data_ptr()
        if side is not None:
            side.wait_stream(main)                           # the inputs were produced on the main stream
        enc_done = []
        for k in range(pieces):                              # encoder pieces, back to back (side stream on the GPU)
            a.fwd_phase, a.fwd_j_lo, a.fwd_j_hi = 1, bounds[k], bounds[k + 1]
            if side is None:
                lib.call("iplan_beh_fwd", a, stream)
            else:
                _launch("beh_enc_fwd_kernel", lambda: lib.call("iplan_beh_fwd", a, side.cuda_stream), stream=side)
                ev = torch.cuda.Event()
                ev.record(side)
                enc_done.append(ev)
        for k in range(pieces):                              # decoder pieces, each behind its encoder piece
            if side is not None:
                main.wait_event(enc_done[k])
            a.fwd_phase, a.fwd_j_lo, a.fwd_j_hi = 2, bounds[k], bounds[k + 1]
            _launch("beh_dec_fwd_kernel", lambda: lib.call("iplan_beh_fwd", a, stream))
        a.fwd_phase, a.fwd_j_lo, a.fwd_j_hi = 3, 0, 0
        lib.call("iplan_beh_fwd", a, stream)
        a.fwd_phase = 0
        if side is not None:
            for k in ("saved_enc", "saved_lat", "enc_carry"):
                out[k].record_stream(side)
            for t in (hist, mask):
                t.record_stream(side)
    out["_args"] = a
    out["_keep"] = (hist, mask, keep, win_norm)
    return out


def beh_window_mask_sums(mask, L_win, hard=False):
    """[n_nets, J] float32: for every window the sum of ``mask`` [n_nets, E, T] over the envs and the window's target
    steps -- what the behaviour kernels sum in-kernel when no ``win_norm`` is given (sums of 0/1 flags: exact)."""
    n_nets, E, T = mask.shape
    col = mask.sum(dim=1)                                  # [n_nets, T]
    if hard:
        J = T // L_win - 1
        return col[:, :J * L_win].sum(dim=1, keepdim=True).expand(n_nets, J).contiguous()
    J = T - 1 - L_win
    cs = torch.cat([torch.zeros(n_nets, 1, dtype=col.dtype, device=col.device), col.cumsum(dim=1)], dim=1)   # cs[k] = sum_{t<k}
    j = torch.arange(J, device=col.device)
    return (cs[:, j + 1 + L_win] - cs[:, j + 1]).contiguous()


def beh_eval(enc_arena, dec_arena, hist, mask, L_win, Z, coef, thres, want_latent=False, want_recon=False, want_sums=True, lib=None):
    """The chain of ``beh_forward`` (soft update) without dropout, forward only, for all nets in one launch: nothing is recorded,
    no seed is drawn, no side stream is used.  hist [n_nets, E, T, N, d] (first three dims may be strided), mask [n_nets, E, T]
    contiguous (only needed, and only read, with ``want_sums``; None otherwise).  Any d + Z <= 16.
    Returns dict(latent [n_nets, E*N, J, Z] = the latent after window j's update, recon [n_nets, E*N, J, L, d] = the decoder's
    output, sums [n_nets, J, L, 2] = per (window, look-ahead step) the masked L1 error sum and the clamped distance sum), None
    for what was not asked for."""
    lib = _lib(lib)
    assert want_latent or want_recon or want_sums, "beh_eval: no output asked for"
    a = L.BehEvalArgs()
    n_nets, E, T, N, d = _enc_rows(a, enc_arena, hist, L_win, Z, coef)
    dev = hist.device
    f32 = dict(dtype=torch.float32, device=dev)
    J = T - 1 - L_win
    rows = E * N
    a.thres = thres
    a.dec_params, a.dec_s_net = dec_arena.data.data_ptr(), dec_arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.dec_off[i] = dec_arena.off(k)
    out = dict(latent=None, recon=None, sums=None)
    part = None
    Jp = max(J, 0)                                         # (J < 1 is refused by the host check of the entry point, before any launch)
    if want_latent:
        out["latent"] = torch.empty(n_nets, rows, Jp, Z, **f32)
        a.latent = out["latent"].data_ptr()
    if want_recon:
        out["recon"] = torch.empty(n_nets, rows, Jp, L_win, d, **f32)
        a.recon = out["recon"].data_ptr()
    if want_sums:
        assert mask is not None and mask.shape == (n_nets, E, T) and mask.is_contiguous() and mask.dtype == torch.float32 and mask.device == dev
        a.mask = mask.data_ptr()
        out["sums"] = torch.empty(n_nets, Jp, L_win, 2, **f32)
        part = torch.empty(n_nets, Jp, L_win, 2, (rows + 15) // 16, **f32)
        a.sums, a.part = out["sums"].data_ptr(), part.data_ptr()
    _launch("beh_eval_kernel", lambda: lib.call("iplan_beh_eval", a, L.current_stream(dev)))
    out["_args"] = a
    out["_keep"] = (hist, mask, part)
    return out


def enc_saliency_scratch_floats(n_nets, rows, windows):
    """floats of caller scratch ``iplan_enc_saliency`` needs: he_j of windows 0 .. max(windows) and one index per slot; independent of K"""
    return n_nets * rows * ((max(windows) + 1) * 32 + len(windows))


ENC_SAL_OUTPUTS = ("grad", "step_l1", "step_gxi", "feature_l1", "carry_l2", "latent", "target_index", "active")


def enc_saliency(enc_arena, hist, windows, K, L_win, Z, coef, seed=None, seed_index=-1, want=("grad",), out=None, lib=None):
    """d <v, lat_j> / d x_{j-r}: BPTT through the behaviour encoder's chain back to the raw history (csrc/enc_saliency.hip), for all
    nets, every (env, entity) chain and every target window j in ``windows`` (sorted, distinct ints in [0, J), J = T - 1 - L_win).
    hist [n_nets, E, T, N, d] (first three dims may be strided); ``K`` earlier windows are unrolled, R = K + L_win; the cotangent v is
    ``seed`` [n_nets, E*N, nW, Z] or, with ``seed=None``, the one-hot of ``seed_index`` (-1: the chain's own argmax of lat_j).
    ``want``: names out of ENC_SAL_OUTPUTS.  Returns a dict with grad [n_nets, E*N, nW, R, d], step_l1 / step_gxi [n_nets, E*N, nW, R],
    feature_l1 [n_nets, E*N, nW, d], carry_l2 [n_nets, E*N, nW], latent [n_nets, E*N, nW, Z], target_index int32 [n_nets, E*N, nW],
    active int32 [n_nets, E*N, nW, K+1, L_win] (a 32-bit mask), None for what was not asked for.  ``out``: optional dict of
    destination tensors of exactly those shapes (contiguous) for some of the wanted names."""
    lib = _lib(lib)
    a = L.EncSaliencyArgs()
    n_nets, E, T, N, d = _enc_rows(a, enc_arena, hist, L_win, Z, coef)
    assert all(k in ENC_SAL_OUTPUTS for k in want), want
    dev = hist.device
    windows, w_host, w_dev = _index_list(a, "windows", windows, dev)
    nW, rows, R = len(windows), E * N, K + L_win
    a.K, a.nW = K, nW
    # the kernel reads steps 0 .. max(windows) of every (net, env): they must lie inside the history's storage
    if nW and 0 <= max(windows) < T and min(hist.stride(0), hist.stride(1), hist.stride(2)) >= 0:
        _inside(hist, (n_nets - 1) * hist.stride(0) + (E - 1) * hist.stride(1) + max(windows) * hist.stride(2) + N * d, "enc_saliency: hist")
    if seed is not None:
        assert seed.dtype == torch.float32 and seed.device == dev and seed.is_contiguous() and seed.shape == (n_nets, rows, nW, Z), seed.shape
        a.seed = seed.data_ptr()
    a.seed_index = int(seed_index)
    floats = enc_saliency_scratch_floats(n_nets, rows, windows) if nW and 0 <= max(windows) < T else 0
    scratch = torch.empty(max(floats, 4), dtype=torch.float32, device=dev)      # (an inspection call: not kept between calls)
    a.scratch, a.scratch_floats = scratch.data_ptr(), floats
    shapes = dict(grad=(R, d), step_l1=(R,), step_gxi=(R,), feature_l1=(d,), carry_l2=(), latent=(Z,), target_index=(), active=(K + 1, L_win))
    res = {k: None for k in ENC_SAL_OUTPUTS}
    for k in want:
        dt = torch.float32 if k not in ("target_index", "active") else torch.int32
        setattr(a, k, _dest(out, res, k, (n_nets, rows, nW) + shapes[k], dt, dev))
    _launch("enc_saliency_kernel", lambda: lib.call("iplan_enc_saliency", a, L.current_stream(dev)))
    res["_args"] = a
    res["_keep"] = (hist, w_host, w_dev, seed, scratch)
    return res


def enc_knockout_windows(J, starts, H):
    """Jn: the windows 0 .. Jn-1 of the base chain that ``iplan_enc_knockout`` walks for these jobs"""
    return min(J, max(starts) + H)


def enc_knockout_workspace_floats(n_nets, rows, J, starts, H):
    """floats of caller workspace ``iplan_enc_knockout`` needs: he_j of the base chain's windows 0 .. Jn-1"""
    return n_nets * rows * enc_knockout_windows(J, starts, H) * 32


ENC_KO_OUTPUTS = ("latent", "intent_base", "latent_ko", "hidden_ko", "intent", "latent_shift_sq", "state_shift_sq")


def enc_knockout(enc_arena, hist, starts, D, H, L_win, Z, coef, columns=None, baseline=None, hold=False,
                 want=("latent", "intent_base", "intent", "latent_shift_sq", "state_shift_sq"), out=None, workspace=None, lib=None):
    """The finite change of the intent latent when the selected ``columns`` (None = all d) of steps s .. s+D-1 of the raw history are
    replaced, for every start s in ``starts`` (sorted, distinct ints in [0, J), J = T - 1 - L_win), every net and every (env, entity)
    chain, over the H windows s .. s+H-1 (csrc/enc_knockout.hip).  hist [n_nets, E, T, N, d] (first three dims may be strided) is read
    in place.  The replacement: ``baseline`` [n_nets, d] (None = zeros) or, with ``hold=True``, the chain's own row of step s-1.
    ``want``: names out of ENC_KO_OUTPUTS ("latent" is always produced).  Returns a dict with latent [n_nets, E*N, Jn, Z] and
    intent_base int32 [n_nets, E*N, Jn] of the base chain (Jn = min(J, max(starts) + H)), latent_ko [n_nets, E*N, Q, H, Z], hidden_ko
    [n_nets, E*N, Q, H, 32], intent int32 [n_nets, E*N, Q, H], latent_shift_sq / state_shift_sq [n_nets, E*N, Q, H]; None for what
    was not asked for.  Slots of windows s + h >= J are zero.  ``out``: optional dict of destination tensors of exactly those shapes
    (contiguous) -- the kernel writes only the slots that exist, so the caller prepares the others; ``workspace``: an optional
    float32 tensor of at least enc_knockout_workspace_floats(...) elements."""
    lib = _lib(lib)
    a = L.EncKnockoutArgs()
    n_nets, E, T, N, d = _enc_rows(a, enc_arena, hist, L_win, Z, coef)
    want = tuple(dict.fromkeys(("latent",) + tuple(want)))
    assert all(k in ENC_KO_OUTPUTS for k in want), want
    dev = hist.device
    starts, s_host, s_dev = _index_list(a, "starts", starts, dev)
    Q, rows, J = len(starts), E * N, T - 1 - L_win
    ok = Q > 0 and J >= 1 and H >= 1 and all(0 <= s < J for s in starts)          # (everything else is refused by the entry point)
    Jn = enc_knockout_windows(J, starts, H) if ok else 0
    a.Q, a.D, a.H = Q, D, H
    # the kernel reads steps 0 .. Jn-1 of every (net, env): they must lie inside the history's storage
    if ok and min(hist.stride(0), hist.stride(1), hist.stride(2)) >= 0:
        _inside(hist, (n_nets - 1) * hist.stride(0) + (E - 1) * hist.stride(1) + (Jn - 1) * hist.stride(2) + N * d, "enc_knockout: hist")
    cols = list(range(d)) if columns is None else [int(c) for c in columns]
    assert all(0 <= c < 32 for c in cols), cols
    a.col_mask = sum(1 << c for c in set(cols))
    a.hold = int(hold)
    if baseline is not None:
        assert baseline.dtype == torch.float32 and baseline.device == dev and baseline.is_contiguous() and baseline.shape == (n_nets, d), baseline.shape
        a.baseline = baseline.data_ptr()
    floats = n_nets * rows * Jn * 32
    if workspace is None:
        workspace = torch.empty(max(floats, 4), dtype=torch.float32, device=dev)   # (an inspection call: not kept between calls)
    else:
        assert workspace.dtype == torch.float32 and workspace.device == dev and workspace.is_contiguous() and workspace.numel() >= floats
    a.workspace, a.workspace_floats = workspace.data_ptr(), floats
    Hs = max(H, 0)
    shapes = dict(latent=(Jn, Z), intent_base=(Jn,), latent_ko=(Q, Hs, Z), hidden_ko=(Q, Hs, 32), intent=(Q, Hs), latent_shift_sq=(Q, Hs),
                  state_shift_sq=(Q, Hs))
    res = {k: None for k in ENC_KO_OUTPUTS}
    for k in want:
        dt = torch.int32 if k in ("intent_base", "intent") else torch.float32
        fresh = torch.empty if k in ("latent", "intent_base") else torch.zeros      # slots of windows past J stay zero
        setattr(a, k, _dest(out, res, k, (n_nets, rows) + shapes[k], dt, dev, fresh=fresh))
    _launch("enc_knockout_kernel", lambda: lib.call("iplan_enc_knockout", a, L.current_stream(dev)))
    res["_args"] = a
    res["_keep"] = (hist, s_host, s_dev, baseline, workspace)
    return res


def beh_backward(enc_arena, dec_arena, fwd, accumulate=False, penalty=0.0, E_norm=0, defer_dec_wgrad=False, lib=None):
    """BPTT of beh_forward's behaviour loss: fills both gradient arenas (``accumulate=True``: adds to them -- launches on
    disjoint env chunks of one batch, normalised by a shared ``win_norm``).
    ``defer_dec_wgrad=True``: the DECODER's weight-gradient contraction is not launched; the returned dict carries
    ``"dec_wgrad"``, a callable ``(stream)`` that enqueues it (one call over all steps) on ``stream`` behind the BPTT.  The
    caller decides where that work runs -- nothing but the decoder's own optimiser step depends on it."""
    lib = _lib(lib)
    a = fwd["_args"]
    n_nets, E, N, T, Lw, d, Z = a.n_nets, a.E, a.N, a.T, a.L, a.d, a.Z
    J, rows = ((T // Lw - 1) if a.hard else (T - 1 - Lw)), E * N
    dev = fwd["loss"].device
    f32 = dict(dtype=torch.float32, device=dev)
    tiles = (rows + 15) // 16
    dd = torch.empty(n_nets, tiles, L.BEH_DSAVE_DEC // 16, J * Lw, 16, 16, **f32)          # column-grouped like saved_dec (beh_forward)
    if rows % 16:
        dd[:, -1, :, :, rows % 16:].zero_()
    dl = torch.empty(n_nets, rows, J, L.BEH_DSAVE_LAT, **f32)
    ep = torch.empty(n_nets, tiles, L.BEH_ENC_PART, **f32)
    a.dsave_dec, a.dsave_lat, a.enc_part = dd.data_ptr(), dl.data_ptr(), ep.data_ptr()
    a.enc_grad, a.enc_grad_s_net = enc_arena.grad.data_ptr(), enc_arena.grad.stride(0)
    a.enc_grad_beta = 1.0 if accumulate else 0.0
    a.penalty, a.E_norm = float(penalty), int(E_norm)      # behavior_variation_penalty: the stability term's weight in the loss
    # decoder BPTT, second form (the default): the thin weight gradients (out.*, linear.*) are accumulated in the kernel and
    # reduced into the arena by its last window range; the first form (IPLAN_DEC_BWD_V1=1) and IPLAN_DEC_THIN_ROWS=1 (A/B knob)
    # stream row gradients to iplan_wgrad instead
    thin = _beh_thin_in_kernel()
    assert thin or not a.fwd_skip_act, "the forward skipped the output layer's input: the row-gradient path needs it"
    tp = None
    if thin:
        tp = torch.empty(n_nets, (tiles + L.BEH_DEC_BWD2_TILES - 1) // L.BEH_DEC_BWD2_TILES, L.BEH_DEC_THIN_PART, **f32)
        a.dec_thin_part, a.dec_grad, a.dec_grad_s_net = tp.data_ptr(), dec_arena.grad.data_ptr(), dec_arena.grad.stride(0)
        a.dec_grad_beta = 1.0 if accumulate else 0.0
    else:
        a.dec_thin_part = None
    SD, DD = L.BEH_SAVE_DEC, L.BEH_DSAVE_DEC
    n_in = J * Lw
    sd = fwd["saved_dec"].data_ptr()
    # rows of the contraction = (chain tile, step * 16 + chain): 16 floats apart inside a column group, groups n_in * 256 apart
    cgs = n_in * 256
    sd_st, dd_st = (tiles * n_in * 16 * SD, n_in * 16 * SD, 16), (tiles * n_in * 16 * DD, n_in * 16 * DD, 16)
    H = 64
    off = dec_arena.off

    def dec_wgrad(s0, s1, beta):
        """decoder weight gradients over the rows of steps [s0, s1) of every chain (accumulating when beta = 1)"""
        w = Wgrad(dec_arena.grad, n_nets, tag="iplan_wgrad:beh_dec")
        ddp, sdp, n = dd.data_ptr() + 4 * s0 * 256, sd + 4 * s0 * 256, (s1 - s0) * 16
        cg = dict(dy_cg_stride=cgs, x_cg_stride=cgs)
        if not thin:
            w.add(ddp, dd_st, d, tiles, n, x=sdp, x_strides=sd_st, K=H, x_col0=416, beta=beta,
                  dw_off=off("decoder.out.weight"), db_off=off("decoder.out.bias"), **cg)
        w.add(ddp, dd_st, 3 * H, tiles, n, x=sdp, x_strides=sd_st, K=H, x_col0=32, beta=beta, seg=(3 * H, 80, 0),
              dw_off=off("decoder.rnn.weight_ih_l0"), db_off=off("decoder.rnn.bias_ih_l0"), **cg)
        # recurrent operand = the previous step's hidden state (16 rows back); the step before a range's first one is still in
        # the record and is read in place, the step before step 0 is zero
        w.add(ddp, dd_st, 3 * H, tiles, n, x=sdp, x_strides=sd_st, K=H, x_col0=352, x_shift=-16, x_pre_valid=s0 > 0, beta=beta,
              dw_off=off("decoder.rnn.weight_hh_l0"), db_off=off("decoder.rnn.bias_hh_l0"), seg=(2 * H, 80, 80 + 3 * H), **cg)
        # input Linear: the record keeps its input row [x_t || latent] as one tile
        if not thin:
            w.add(ddp, dd_st, H, tiles, n, x=sdp, x_strides=sd_st, K=d + Z, beta=beta, seg=(H, 16, 0),
                  dw_off=off("decoder.linear.weight"), db_off=off("decoder.linear.bias"), **cg)
        w._keep += [dd, fwd, tp]
        w.run(lib)

    # Pipeline: the decoder BPTT runs in pieces (top windows first) on the main stream; the weight-gradient contraction
    # of the rows a piece produced and the encoder's BPTT over the same windows (it needs their d(loss)/d(latent)) run
    # on two side streams beside the next decoder piece (the decoder kernel holds 138 of the 256 CUs).
    side = side2 = None
    if dev.type == "cuda" and not os.environ.get("IPLAN_BEH_SERIAL"):       # (the knob is for kernel timing experiments)
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev, main.cuda_stream)
        side2 = _side_stream(dev, main.cuda_stream, 2)
    if defer_dec_wgrad and side is None and dev.type == "cuda":
        main = torch.cuda.current_stream(dev)
    pieces = max(1, min(_beh_pieces("BWD", 6 if side is not None else 1), J))
    bounds = _piece_bounds(J, pieces)
    if thin:
        # the in-kernel thin gradients exist in the BPTT's second form only, which takes at most BEH_D2_MAX_WINDOWS windows per launch
        # (iplan_beh_bwd returns EINVAL beyond): episodes longer than that get more pieces instead of failing
        while max(b1 - b0 for b0, b1 in zip(bounds[:-1], bounds[1:])) > L.BEH_D2_MAX_WINDOWS:
            pieces += 1
            bounds = [round(J * k / pieces) for k in range(pieces + 1)]
    pieces = len(bounds) - 1
    carry = torch.empty(n_nets, tiles, 2, 512, **f32)
    ecarry = torch.empty(n_nets, tiles, 768, **f32)
    a.dec_carry, a.enc_carry = carry.data_ptr(), ecarry.data_ptr()
    stream = L.current_stream(dev)
    for k in range(pieces, 0, -1):
        a.bwd_phase, a.bwd_j_lo, a.bwd_j_hi = 1, bounds[k - 1], bounds[k]
        _launch("beh_dec_bwd_kernel", lambda: lib.call("iplan_beh_bwd", a, stream))
        beta = 0.0 if (k == pieces and not accumulate) else 1.0
        if side is None:
            if not defer_dec_wgrad:
                dec_wgrad(bounds[k - 1] * Lw, bounds[k] * Lw, beta)
            a.bwd_phase = 2
            lib.call("iplan_beh_bwd", a, stream)
        else:
            ev = torch.cuda.Event()
            ev.record(main)
            side2.wait_event(ev)
            if not defer_dec_wgrad:
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    dec_wgrad(bounds[k - 1] * Lw, bounds[k] * Lw, beta)
            a.bwd_phase = 2
            _launch("beh_enc_bwd_kernel", lambda: lib.call("iplan_beh_bwd", a, side2.cuda_stream), stream=side2)
    a.bwd_phase, a.bwd_j_lo, a.bwd_j_hi = 0, 0, 0
    out = dict(dsave_dec=dd, dsave_lat=dl, enc_part=ep, dec_thin_part=tp)
    if defer_dec_wgrad:
        ev_bptt = None
        if dev.type == "cuda":
            ev_bptt = torch.cuda.Event()
            ev_bptt.record(main)                                         # every decoder BPTT range is behind this

        def run_dec_wgrad(strm=None):
            if strm is None or dev.type != "cuda":
                dec_wgrad(0, J * Lw, 1.0 if accumulate else 0.0)
                return
            strm.wait_event(ev_bptt)
            # ... and behind whatever the caller has enqueued on the main stream by now (Behavior_policy.learn: the encoder's
            # BPTT tail, gradient reduction and optimiser step -- what the next rollout waits for).  The wide contraction's
            # 372-register waves take whole CUs: started right behind the last decoder range it ran beside the encoder's last
            # range and stretched it from 0.6 to 3.9 ms (rocprofv3 trace, profiles/r03c_notes.md).
            ev_now = torch.cuda.Event()
            ev_now.record(torch.cuda.current_stream(dev))
            strm.wait_event(ev_now)
            with torch.cuda.stream(strm):
                dec_wgrad(0, J * Lw, 1.0 if accumulate else 0.0)
            for t in (dd, fwd["saved_dec"]):
                t.record_stream(strm)
        out["dec_wgrad"] = run_dec_wgrad
    if side is not None:
        for st in ((side2,) if defer_dec_wgrad else (side, side2)):
            ev_done = torch.cuda.Event()
            ev_done.record(st)
            main.wait_event(ev_done)
        if not defer_dec_wgrad:
            for t in (dd, carry, fwd["saved_dec"]):                     # touched by the side streams: keep the allocator honest
                t.record_stream(side)
        for t in (dl, ep, ecarry, fwd["saved_enc"], fwd["saved_lat"]):
            t.record_stream(side2)
    return out


def bdec_forward(enc_arena, dec_arena, window, latent, hidden, drop_p=0.0, keep=None, seed=0, lib=None):
    """Behavior_Latent_Decoder.forward on one explicit window for all nets (single-window mode of iplan_beh_fwd).
    window [n_nets, rows, L, d], latent [n_nets, rows, Z], hidden [n_nets, rows, 64] -> (pred [n_nets, rows, L, d],
    new hidden [n_nets, rows, 64])."""
    lib = _lib(lib)
    n_nets, rows, Lw, d = window.shape
    Z = latent.shape[-1]
    dev = window.device
    f32 = dict(dtype=torch.float32, device=dev)
    for t in (window, latent, hidden):
        assert t.is_contiguous() and t.dtype == torch.float32
    a = L.BehArgs()
    a.n_nets, a.E, a.N, a.T, a.L, a.d, a.Z = n_nets, rows, 1, Lw + 2, Lw, d, Z
    a.win, a.lat_in, a.hd_in = window.data_ptr(), latent.data_ptr(), hidden.data_ptr()
    pred, hout = torch.empty(n_nets, rows, Lw, d, **f32), torch.empty(n_nets, rows, 64, **f32)
    saved = torch.empty(n_nets, (rows + 15) // 16 * 16, 1, Lw, L.BEH_SAVE_DEC, **f32)        # (scratch record: column-grouped by chain tile)
    a.pred_out, a.hd_out, a.saved_dec = pred.data_ptr(), hout.data_ptr(), saved.data_ptr()
    if keep is not None:
        assert keep.dtype == torch.uint8 and keep.shape == (n_nets, 1, rows, Lw, 64) and keep.is_contiguous()
        a.keep = keep.data_ptr()
    a.seed, a.drop_p, a.coef, a.thres = seed, drop_p, 0.0, 0.0
    a.enc_params, a.enc_s_net = enc_arena.data.data_ptr(), enc_arena.net_stride
    for i, k in enumerate(L.ENC_PARAM_ORDER):
        a.enc_off[i] = enc_arena.off(k)
    a.dec_params, a.dec_s_net = dec_arena.data.data_ptr(), dec_arena.net_stride
    for i, k in enumerate(L.DEC_PARAM_ORDER):
        a.dec_off[i] = dec_arena.off(k)
    lib.call("iplan_beh_fwd", a, L.current_stream(dev))
    return pred, hout


# ---- FC behaviour ablation: stacked three-layer perceptrons -------------------------------------------------
MLP3_PARAM_ORDER = ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "out.weight", "out.bias")


def mlp3_forward(arena, prefix, x, H, O, softmax=False, target=None, save=True, lib=None):
    """out = [softmax](W3 tanh(W2 tanh(W1 x + b1) + b2) + b3) for all nets: x [n_nets, rows, K0] -> out [n_nets, rows, O].
    ``prefix``: parameter-name prefix inside the arena ("" or "decoder.").  With ``target`` also returns the per-net sum of
    |target - out| (L1 numerator).  Returns dict(out, saved, l1, _args)."""
    lib = _lib(lib)
    n_nets, rows, K0 = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32
    dev = x.device
    f32 = dict(dtype=torch.float32, device=dev)
    a = L.Mlp3Args()
    a.n_nets, a.K0, a.H, a.O, a.softmax, a.rows = n_nets, K0, H, O, 1 if softmax else 0, rows
    a.x, a.params, a.params_s_net = x.data_ptr(), arena.data.data_ptr(), arena.net_stride
    for i, k in enumerate(MLP3_PARAM_ORDER):
        a.off[i] = arena.off(prefix + k)
    out = dict(out=torch.empty(n_nets, rows, O, **f32))
    a.out = out["out"].data_ptr()
    if save:
        out["saved"] = torch.empty(n_nets, rows, 2 * H, **f32)
        a.saved = out["saved"].data_ptr()
    if target is not None:
        assert target.shape == (n_nets, rows, O) and target.is_contiguous()
        part = torch.empty(n_nets, 4 * ((rows + 63) // 64), **f32)
        a.target, a.loss_part = target.data_ptr(), part.data_ptr()
    lib.call("iplan_mlp3_fwd", a, L.current_stream(dev))
    if target is not None:
        out["l1"] = part.sum(dim=1)
    out["_args"] = a
    out["_keep"] = (x, target)
    return out


def mlp3_backward(arena, prefix, fwd, g_out=None, g_scale=0.0, want_dx=False, beta=0.0, lib=None):
    """Backward of mlp3_forward: fills the arena's gradient entries of the six tensors (accumulating when beta = 1) and
    returns dx [n_nets, rows, K0] if asked.  d(out) = g_out, or the L1 loss's -sign(target - out) * g_scale."""
    lib = _lib(lib)
    a = fwd["_args"]
    n_nets, rows, K0, H, O = a.n_nets, a.rows, a.K0, a.H, a.O
    dev = fwd["out"].device
    f32 = dict(dtype=torch.float32, device=dev)
    O16 = 16 * ((O + 15) // 16)
    DS = 2 * H + O16
    ds = torch.empty(n_nets, rows, DS, **f32)
    a.dsave = ds.data_ptr()
    dx = torch.empty(n_nets, rows, K0, **f32) if want_dx else None
    a.dx = dx.data_ptr() if want_dx else None
    if g_out is not None:
        assert g_out.shape == (n_nets, rows, O) and g_out.is_contiguous()
        a.g_out = g_out.data_ptr()
    else:
        a.g_out, a.g_scale = None, g_scale
    lib.call("iplan_mlp3_bwd", a, L.current_stream(dev))
    off = arena.off
    sv, x = fwd["saved"], fwd["_keep"][0]
    w = Wgrad(arena.grad, n_nets)
    dst = (rows * DS, DS, DS)
    w.add(ds.data_ptr(), dst, H, rows, 1, x=x.data_ptr(), x_strides=(rows * K0, K0, K0), K=K0, beta=beta,
          dw_off=off(prefix + "linear_1.weight"), db_off=off(prefix + "linear_1.bias"))
    w.add(ds.data_ptr() + 4 * H, dst, H, rows, 1, x=sv.data_ptr(), x_strides=(rows * 2 * H, 2 * H, 2 * H), K=H, beta=beta,
          dw_off=off(prefix + "linear_2.weight"), db_off=off(prefix + "linear_2.bias"))
    w.add(ds.data_ptr() + 8 * H, dst, O, rows, 1, x=sv.data_ptr() + 4 * H, x_strides=(rows * 2 * H, 2 * H, 2 * H), K=H, beta=beta,
          dw_off=off(prefix + "out.weight"), db_off=off(prefix + "out.bias"))
    w._keep += [ds, sv, x]
    w.run(lib)
    return dx
