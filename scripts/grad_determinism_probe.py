"""Is one training step of the fused ResNet-50 bitwise reproducible in its gradients?  Runs
the same step (same weights, same batch, backends already picked, no optimizer update)
twice and compares every parameter gradient -- one JSON line per differing parameter in
BACKWARD order (the classifier first: the first line names where the two backward passes
part), then a summary with the input-gradient backends of the stride-2 3x3 layers.
``BATCH=n`` sets the batch size (default 32), ``DETERMINISTIC=1`` runs under
``torch.use_deterministic_algorithms(True, warn_only=True)``."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ray_lightning_accelerators_amd.models.resnet import resnet50  # noqa: E402
from ray_lightning_accelerators_amd.ops import conv as C  # noqa: E402
from ray_lightning_accelerators_amd.parallel.arena import ParamArena  # noqa: E402


def main():
    B = int(os.environ.get("BATCH", "32"))
    deterministic = os.environ.get("DETERMINISTIC", "0") == "1"
    if deterministic:  # what Trainer(deterministic=True) sets
        torch.use_deterministic_algorithms(True, warn_only=True)
    dev = torch.device("cuda", 0)
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(0)
    m = resnet50(fused_bn=True).to(dev).to(memory_format=torch.channels_last)
    arena = ParamArena(m)
    arena.enable_bf16_shadow(m)
    g = torch.Generator(device=dev).manual_seed(1)
    xb = torch.randn(B, 3, 224, 224, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    yb = torch.randint(0, 1000, (B,), device=dev, generator=g)
    calls = {"s2_dgrad_hip": 0, "miopen_bwd_dx": 0}
    real_hip, real_bwd = C.conv3x3s2_dgrad_hip, C._miopen_bwd

    def hip(*a):
        calls["s2_dgrad_hip"] += 1
        return real_hip(*a)

    def bwd(dy, x, w4, stride, padding, need_dx, need_dw):
        calls["miopen_bwd_dx"] += bool(need_dx)
        return real_bwd(dy, x, w4, stride, padding, need_dx, need_dw)

    C.conv3x3s2_dgrad_hip, C._miopen_bwd = hip, bwd
    # running statistics move with every training forward: both compared steps start from this state
    state = {k: v.clone() for k, v in m.state_dict().items()}

    def step():
        m.load_state_dict(state)
        arena.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(xb)
        F.cross_entropy(out.float(), yb).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    step()  # backend picks
    calls.update(s2_dgrad_hip=0, miopen_bwd_dx=0)
    g1 = step()
    per_step = dict(calls)
    g2 = step()
    names = [n for n, _ in m.named_parameters() if n in g1][::-1]  # backward order
    differing = [n for n in names if not torch.equal(g1[n], g2[n])]
    for n in differing[:12]:
        d = (g1[n].float() - g2[n].float()).abs()
        print(json.dumps({"parameter": n, "shape": list(g1[n].shape), "max_abs_diff": float(d.max()),
                          "n_diff": int((d > 0).sum()), "numel": g1[n].numel()}), flush=True)
    print(json.dumps({"parameters": len(names), "differing": len(differing), "batch": B,
                      "deterministic": deterministic, "first_in_backward_order": differing[0] if differing else None,
                      "calls_per_step": per_step,
                      "picks": {k: v["pick"] for k, v in C.choices().items()
                                if k.startswith("dgrad_s2") or k.startswith("fwd_kxk")}}), flush=True)


if __name__ == "__main__":
    main()
