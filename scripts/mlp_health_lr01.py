"""How often the fused MNIST step's 12.20 clamp fires at the reference's default learning
rate (0.1, Adam), and what the loss does there.

Two full epochs of the bench's synthetic task (55,000 samples, batch 32) at 784-32-64-10
and at the 128-256 corner.  Per shape: ``FusedMLPEngine.health()`` after the run (hipGraph
replays), the 20-step window in which the counts first move (an eager twin, read every 20
steps), the loss of the last 200 steps, and the same figure for fp32 nn.Linear math +
torch.optim.Adam on the CPU (three initial seeds at 32-64: their spread is the margin ``m``)
and for bf16 autocast on the GPU, all from the same initial weights and batch order.  Loss
curves are kept as 100-step means.

    python scripts/mlp_health_lr01.py OUT.json
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_lightning_accelerators_amd.config import get_config, set_config  # noqa: E402
from ray_lightning_accelerators_amd.models.data import synthetic_mnist  # noqa: E402
from ray_lightning_accelerators_amd.ops import fused_mlp  # noqa: E402
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices  # noqa: E402

NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
B, LR, LAST = 32, 0.1, 200
DEV = torch.device("cuda", 0)


def torch_run(p_init, L1, L2, n_steps, x, y, autocast, order_seed=0):
    """fp32 nn.Linear math + torch.optim.Adam on the engine's batches (CPU, fp32), or the same
    under bf16 autocast on the GPU; every step's loss."""
    dev = DEV if autocast else torch.device("cpu")
    p = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in
         zip(NAMES, fused_mlp.mlp_unpack(p_init.float(), L1, L2).values())}
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    xd, yd = x.to(dev), y.to(dev)
    nb = x.size(0) // B
    losses, order = [], None
    for s in range(n_steps):
        epoch, cur = divmod(s, nb)
        if cur == 0:
            order = shard_indices(x.size(0), 1, 0, epoch, order_seed, True).to(dev)
        idx = order[cur * B:(cur + 1) * B]
        xb = xd[idx].float() / 255.0
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            h = torch.relu(F.linear(xb, p["W1"], p["b1"]))
            h = torch.relu(F.linear(h, p["W2"], p["b2"]))
            z = F.linear(h, p["W3"], p["b3"])
        loss = F.nll_loss(torch.log_softmax(z.float(), 1), yd[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses).cpu().tolist()


def means(c, k=100):
    return [sum(c[i:i + k]) / len(c[i:i + k]) for i in range(0, len(c), k)]


def last(c):
    return sum(c[-LAST:]) / LAST


def main(out_path):
    set_config(get_config().replace(mlp_saturation="ignore"))
    x, y = synthetic_mnist(55000, seed=0)
    n = 2 * (x.size(0) // B)
    res = {"steps": n, "batches_per_epoch": x.size(0) // B, "lr": LR, "batch": B}
    for L1, L2 in ((32, 64), (128, 256)):
        eng = FusedMLPEngine(L1, L2, B, lr=LR, device=DEV, seed=0)
        eng.set_data(x, y)
        p_init = eng.params.detach().cpu().clone()
        assert eng.capture(8)
        eng.run(n - 1)
        torch.cuda.synchronize()
        w1 = fused_mlp.mlp_unpack(eng.params.cpu(), L1, L2)["layer_1.weight"]
        r = {"health": eng.health(), "loss_fused_last200": eng.recent_stats(LAST)[:, 0].mean().item(),
             "state_finite": all(bool(torch.isfinite(getattr(eng, k)).all())
                                 for k in ("params", "exp_avg", "exp_avg_sq")),
             "w1_absmax": w1.abs().max().item(), "w1_absmean": w1.abs().mean().item()}
        # eager twin, one launch per step: when the counts first move, how they grow, the loss curve
        twin = FusedMLPEngine(L1, L2, B, lr=LR, device=DEV, seed=0)
        twin.set_data(x, y)
        first_sat = first_bad = None
        series, curve = [], []
        for s in range(1, n + 1):
            twin.run(1)
            if s % 20 == 0 or s == n:
                h = twin.health()
                if first_sat is None and h["saturated"]:
                    first_sat = (s - 19, s)
                if first_bad is None and h["nonfinite"]:
                    first_bad = (s - 19, s)
                if s % 200 == 0 or s == n:
                    series.append((s, h["saturated"], h["nonfinite"], h["last_step"]))
            if s % 1000 == 0 or s == n:
                curve.extend(twin.recent_stats(1000 if s % 1000 == 0 else s % 1000)[:, 0].tolist())
        r["eager_twin_health"] = twin.health()
        r["eager_twin_params_equal"] = bool(torch.equal(twin.params, eng.params))
        r["first_saturated_in_steps"], r["first_nonfinite_in_steps"] = first_sat, first_bad
        r["series_step_sat_nonfinite_last"] = series
        r["fused_curve_100"] = means(curve)
        r["loss_fp32_last200_by_seed"] = {}
        for sd in ((0, 1, 2) if (L1, L2) == (32, 64) else (0,)):
            pi = p_init if sd == 0 else fused_mlp.init_mlp_params(L1, L2, torch.Generator().manual_seed(sd))
            c = torch_run(pi, L1, L2, n, x, y, autocast=False)
            r["loss_fp32_last200_by_seed"][sd] = last(c)
            if sd == 0:
                r["fp32_curve_100"] = means(c)
        c = torch_run(p_init, L1, L2, n, x, y, autocast=True)
        r["loss_autocast_last200"], r["autocast_curve_100"] = last(c), means(c)
        v = list(r["loss_fp32_last200_by_seed"].values())
        r["fp32_seed_spread"] = max(v) - min(v)
        r["abs_fused_minus_fp32"] = abs(r["loss_fused_last200"] - v[0])
        r["abs_autocast_minus_fp32"] = abs(r["loss_autocast_last200"] - v[0])
        res[f"{L1}-{L2}"] = r
        print(f"{L1}-{L2}", json.dumps({k: val for k, val in r.items() if "curve" not in k and "series" not in k}),
              flush=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "mlp_health_lr01.json")
