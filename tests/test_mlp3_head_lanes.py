"""Lane map of the v3 head's softmax section (csrc/mlp_step3.hip).

The softmax section runs one (batch row, class slot) element per thread and parks
each row's loss statistics in LDS for a reduction off the critical path; it may not
change a bit of the step.  Closed-form cases pin the arg-max tie rule, the empty
class slots, rows without a label and the dZ lane map; a one-launch against
two-launch run with a learning-rate change and weight decay pins the optimizer
epilogues that consume its outputs, bit for bit.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

gpu = pytest.mark.gpu

L1, L2 = 32, 64
B3_CASES = {
    # logits == b3 on every row (layer_3.weight = 0): (b3, the class every row predicts)
    "zero": ([0.0] * 10, 0),  # ten-way tie: the lowest index
    "one_high": ([0.0] * 9 + [4.0], 9),  # the last class slot in use
    "tie_3_7": ([0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0], 3),  # two-way tie: the lower index
}


def _rel(a, b):
    return (a.float() - b.float()).norm().item() / max(b.float().norm().item(), 1e-12)


def _dev():
    return torch.device("cuda", 0)


@gpu
@pytest.mark.parametrize("B", [1, 17, 32, 33])
@pytest.mark.parametrize("case", sorted(B3_CASES))
def test_mlp3_softmax_closed_form(case, B):
    """Logits are exactly b3 on every row, so count / correct are exact and the loss and
    the b3 gradient have closed forms.  B <= 32 runs the one-launch step, B = 33 the
    two-launch head (its second row block holds one valid row).

    The data set holds five batches (labels arange(5 B) % 10) and the step consumes
    the first batch of epoch 0's shuffled order.  A data set of exactly one batch has
    perfectly balanced labels, and at b3 = 0 the expected gradient 0.1 - k_j / B then
    cancels to a quarter of its terms: rounding dZ to bf16 (half an ulp, 2^-9, per
    element) alone can then move it by 2.5e-2 (B = 33) or 2.8e-2 (B = 32) of its norm,
    past the bf16 bound whatever the kernel does.  The rounding-only worst case of the
    batch in use is asserted below, from the labels alone, before the kernel's result
    is looked at.
    """
    dev = _dev()
    b3_list, pred = B3_CASES[case]
    b3 = torch.tensor(b3_list, dtype=torch.float32)
    n = 5 * B
    x = torch.randint(0, 256, (n, 784), generator=torch.Generator().manual_seed(B), dtype=torch.uint8)
    labels = torch.arange(n) % 10
    y = labels[shard_indices(n, 1, 0, 0, 0, True)[:B]]  # the batch the first step consumes (engine seed 0)
    delta = torch.softmax(b3.double(), 0)[None, :] - F.one_hot(y, 10).double()  # B * dZ, exact
    ref = delta.mean(0)
    rounding = 2.0 ** -9 * delta.abs().mean(0).norm().item() / ref.norm().item()
    assert rounding < 1e-2, rounding  # the check is well conditioned: bf16 dZ alone stays inside half the bound
    assert B < 17 or int((y == pred).sum()) > 0  # the predicted class occurs: `correct` below is not trivially 0
    flat = fused_mlp.init_mlp_params(L1, L2, torch.Generator().manual_seed(1))
    views = fused_mlp.mlp_unpack(flat, L1, L2)
    views["layer_3.weight"].zero_()
    views["layer_3.bias"].copy_(b3)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-3, device=dev)
    assert eng.one_launch == (B <= 32)
    eng.set_data(x, labels)
    eng.load_params(flat)
    eng.step()
    torch.cuda.synchronize()
    eng.check()
    st = eng.recent_stats(1)[0].cpu()
    loss, correct, count = float(st[0]), int(st[1]), int(st[2])
    print(f"{case} B={B}: loss {loss:.6f} correct {correct} count {count}")
    assert count == B
    assert correct == int((y == pred).sum())
    want = float(torch.logsumexp(b3.double(), 0) - b3.double()[y].mean())
    print(f"  closed-form loss {want:.6f}")
    assert abs(loss - want) < 3e-2 * max(1.0, loss)
    # the first step's exp_avg is (1 - beta1) * gradient: d loss / d b3 = mean(softmax - onehot)
    nb3 = fused_mlp.mlp_param_count(L1, L2) - 10
    g = eng.exp_avg[nb3:].cpu().double() / (1.0 - eng.betas[0])
    err = _rel(g, ref)
    print(f"  b3 gradient rel err {err:.5f}")
    assert math.isfinite(err) and err < 2e-2, (g.tolist(), ref.tolist())


@gpu
@pytest.mark.parametrize("L1_,L2_,B,wd", [(32, 64, 32, 0.0), (64, 128, 17, 0.0), (32, 64, 32, 1e-2)])
def test_mlp3_one_launch_matches_two_launch_lr_change_and_decay(L1_, L2_, B, wd):
    """Six steps, the learning rate changed between steps 2 and 3, once with weight
    decay: the one-launch step (every block replays the head pass, block 0 reduces the
    parked loss statistics) against the two-launch step -- every state tensor bit
    for bit."""
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    n = 2 * B + B // 2 + 3
    x = torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g)
    a = FusedMLPEngine(L1_, L2_, B, lr=1e-2, weight_decay=wd, device=dev)
    b = FusedMLPEngine(L1_, L2_, B, lr=1e-2, weight_decay=wd, device=dev)
    assert a.one_launch
    b.one_launch = False
    a.set_data(x, y)
    b.set_data(x, y)
    for s in range(6):
        if s == 2:
            a.set_lr(3e-3)
            b.set_lr(3e-3)
        a.step()
        b.step()
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(a.counters[:10].cpu(), b.counters[:10].cpu()), (a.counters, b.counters)
    for k in ("params", "exp_avg", "exp_avg_sq", "shadow", "h1pre", "stats", "xring"):
        pa, pb = getattr(a, k).float(), getattr(b, k).float()
        bad = (pa != pb).nonzero()
        assert bad.numel() == 0, (k, bad.size(0), bad[:8].flatten().tolist(), (pa - pb).abs().max().item())
