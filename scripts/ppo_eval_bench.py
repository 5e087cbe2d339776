"""Times iplan_ppo_eval beside the two launches that form the same five loss numbers in train() -- iplan_ppo_prepare (with its own
advantage normalisation) + iplan_ppo_loss -- on synthetic per-row inputs at config 3's PPO batch (5 agents x 255 episodes x 90 steps
= 22 950 rows each), HIP events around each candidate, the candidates alternating in one process.
Usage: python scripts/ppo_eval_bench.py        (PE_AGENTS / PE_EPISODES / PE_STEPS change the shape)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from iplan_amd import _lib as L  # noqa: E402
from iplan_amd import ops  # noqa: E402

nA, bs, T = (int(os.environ.get(k, v)) for k, v in (("PE_AGENTS", "5"), ("PE_EPISODES", "255"), ("PE_STEPS", "90")))
rows = bs * T
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)  # noqa: E731
reward, v_all = rnd(bs, T + 1, nA, 1), rnd(nA, bs, T + 1)
term = (torch.rand(bs, T + 1, nA, 1, generator=gen) < 0.05).to(torch.uint8).to(dev)
logp = -1.2 + 0.5 * rnd(nA, rows)
old_logp = logp - 0.2 * rnd(nA, rows)
entropy, values = 1.0 + 0.1 * rnd(nA, rows), rnd(nA, rows)
lib = L.get_lib()
stream = torch.cuda.current_stream().cuda_stream


def prepare(skip_norm):
    pp = L.PpoPrepareArgs()
    pp.n_agents, pp.bs, pp.T = nA, bs, T
    pp.reward, pp.rw_s_net, pp.rw_s_ep, pp.rw_s_t = reward.data_ptr(), reward.stride(2), reward.stride(0), reward.stride(1)
    pp.terminated, pp.tm_s_net, pp.tm_s_ep, pp.tm_s_t = term.data_ptr(), term.stride(2), term.stride(0), term.stride(1)
    pp.values, pp.gamma, pp.lam = v_all.data_ptr(), 0.99, 0.95
    outs = [torch.empty(nA, rows, device=dev) for _ in range(4)]
    pp.returns, pp.adv, pp.mask, pp.value_preds = (o.data_ptr() for o in outs)
    pp.skip_norm = skip_norm
    return pp, dict(zip(("returns", "adv", "mask", "value_preds"), outs))


pp_raw, raw = prepare(1)
pp_norm, normed = prepare(0)
lib.call("iplan_ppo_prepare", pp_raw, stream)
parts = min(64, rows // 1024)
msum = torch.empty(nA, device=dev)
pl = L.PpoLossArgs()
pl.n_agents, pl.rows, pl.row_stride = nA, rows, rows
pl.logp, pl.entropy, pl.values, pl.old_logp = logp.data_ptr(), entropy.data_ptr(), values.data_ptr(), old_logp.data_ptr()
pl.adv, pl.value_preds, pl.returns, pl.mask = (normed[k].data_ptr() for k in ("adv", "value_preds", "returns", "mask"))
pl.clip, pl.huber_delta, pl.value_loss_coef, pl.n_parts = 0.2, 10.0, 1.0, parts
g1, g2, st = torch.empty(nA, rows, device=dev), torch.empty(nA, rows, device=dev), torch.zeros(nA, max(parts, 1), 8, device=dev)
pl.g_logp, pl.g_values, pl.stats, pl.mask_sum = g1.data_ptr(), g2.data_ptr(), st.data_ptr(), msum.data_ptr()


def run_train_pair():
    lib.call("iplan_ppo_prepare", pp_norm, stream)
    msum.copy_(normed["mask"].sum(1))
    lib.call("iplan_ppo_loss", pl, stream)


def run_eval(n_parts):
    return ops.ppo_eval(logp, entropy, values, old_logp, raw["adv"], raw["value_preds"], raw["returns"], raw["mask"], T, n_parts=n_parts)


def passes(fn, n_pass=5, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_pass):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return out


run_train_pair()
ev = run_eval(parts)
torch.cuda.synchronize()
print("stats 0-4, eval vs loss kernel: max |difference|", (ev["stats"][:, :5] - st.sum(1)[:, :5]).abs().max().item(), flush=True)
res = {"prepare + mask sum + loss": [], "ppo_eval n_parts=1": [], f"ppo_eval n_parts={parts}": [], "ppo_eval n_parts=256": []}
for _ in range(2):                                         # the candidates alternate, so a drift of the box hits all of them
    res["prepare + mask sum + loss"] += passes(run_train_pair)
    res["ppo_eval n_parts=1"] += passes(lambda: run_eval(1))
    res[f"ppo_eval n_parts={parts}"] += passes(lambda: run_eval(parts))
    res["ppo_eval n_parts=256"] += passes(lambda: run_eval(256))
for k, v in res.items():
    v = sorted(v)
    med = v[len(v) // 2]
    print(f"{k:28s} nA={nA} rows={rows}: median {med:.1f} us  min {v[0]:.1f}  max {v[-1]:.1f}  spread {(v[-1] - v[0]) / med * 100:.1f} %", flush=True)
