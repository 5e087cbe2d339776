"""Time of one ``Prediction_policy.attention_saliency_trace`` call beside the by-hand route of the one-step methods
(``attention_trace`` + lags + 1 ``attention_saliency`` calls on shifted slices, the carries as tensor targets, one read-back).
Config 3's shape: 5 nets, 32 environments, 55 entities; S = 20 steps, targets = the last 8, lags = 10, deterministic, want=("pair",).
Both routes in one process, alternating, device events around each call: median, min and max of ``--rounds`` after ``--warmup``
rounds, per workspace size; the chunk counts and the largest device allocation of each route beside them.  One JSON line per
workspace size.  No threshold is set.

    python scripts/bench_attention_saliency_trace.py [--envs 32] [--steps 20] [--targets 8] [--lags 10] [--rounds 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
from unittest import mock

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--targets", type=int, default=8)
    ap.add_argument("--lags", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workspaces", type=float, nargs="+", default=[256, 8192])
    o = ap.parse_args()
    from iplan_amd import ops
    from iplan_amd.config import default_args
    from iplan_amd.nova.prediction_policy import Prediction_policy

    class Log:
        def log_stat(self, *a, **k):
            pass
    args = default_args("highway", use_cuda=True)
    torch.manual_seed(0)
    pol = Prediction_policy(args, Log())
    E, S, K = o.envs, o.steps, o.lags
    nA, N, d, Z, A = args.n_agents, args.max_vehicle_num, args.obs_shape_single, args.latent_dim, args.attention_dim
    tg = list(range(S - o.targets, S))
    hist = (torch.rand(E, S, nA, N, d) * 2 - 1).cuda()
    hist[..., 0] = 1.0
    beh = torch.softmax(torch.randn(E, S, nA, N, Z), -1).cuda()
    h0 = (torch.randn(E, nA, N, A) * 0.1).cuda()

    def method(mb):
        return pol.attention_saliency_trace(hist, beh, hidden0=h0, lags=K, targets=tg, max_workspace_mb=mb)["lag_l1"]

    def by_hand(mb):
        tr = pol.attention_trace(hist, beh, hidden0=h0, deterministic=True, want=(), _stats=False)
        hid = torch.cat([h0[:, None], tr["latent"][:, :-1]], 1)
        cot, sums = "self", []
        for k in range(K + 1):
            steps = [s - k for s in tg if s - k >= 0]
            one = pol.attention_saliency(hist[:, steps], beh[:, steps], hidden=hid[:, steps], target=cot, max_workspace_mb=mb)
            cot = one["hidden_grad"][:, -len([s for s in tg if s - k - 1 >= 0]):] if k < K else None
            sums.append(one["pair_gl1"].sum(dim=(0, 1, 3, 4)))
        return torch.stack(sums).cpu()                                            # ONE read-back

    def timed(fn, mb):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn(mb)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), (torch.cuda.max_memory_allocated() - base) / (1 << 20)

    for mb in o.workspaces:
        counts = {}
        for name, fn in (("method", method), ("by_hand", by_hand)):
            calls = {"fwd": 0}
            real = ops.gat_forward

            def fwd(*a, _real=real, _calls=calls, **k):
                _calls["fwd"] += 1
                return _real(*a, **k)
            with mock.patch.object(ops, "gat_forward", fwd):
                fn(mb)
            counts[name] = calls["fwd"]                                            # one training-form forward per chunk
        times = {"method": [], "by_hand": []}
        peak = {"method": 0.0, "by_hand": 0.0}
        for r in range(o.warmup + o.rounds):
            for name, fn in (("method", method), ("by_hand", by_hand)):
                ms, mem = timed(fn, mb)
                if r >= o.warmup:
                    times[name].append(ms)
                    peak[name] = max(peak[name], mem)
        out = {"max_workspace_mb": mb, "shape": dict(nets=nA, envs=E, N=N, S=S, targets=len(tg), lags=K), "rounds": o.rounds}
        for name in times:
            out[name] = dict(median_ms=round(statistics.median(times[name]), 3), min_ms=round(min(times[name]), 3), max_ms=round(max(times[name]), 3),
                             chunks=counts[name], peak_alloc_mb=round(peak[name], 1))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
