"""References and bounds of the fused MNIST step's gradient clipping: the fixed-order
norm partials (csrc/optim_kernels.hip ``clip_partials_kernel``, mirrored in torch by
``ops.optim.clip_partials``) and the coefficient the ADAM tail derives from them
(csrc/mlp_step3.hip ``tail_clip_coef``).  Shared by tests/test_clip_reference.py (CPU) and
tests/test_mlp3_clip.py (GPU); nothing here reads an output to decide a tolerance.

Bound of the partials.  Every addend x^2 is >= 0, so each intermediate sum is at most the
total S and a chain of k fp32 roundings is off by at most (k + 1) U S (the "+ 1" covers the
second-order terms, as in tests/optim_reference.py).  From the kernel, one x^2 passes

    1           its square (0 when ``a += x * x`` contracts to an fma: the count covers both)
    passes      ``a_c +=`` once per pass of its thread over the block's slice,
                passes = ceil(ceil((n / 4) / nblk) / 256)
    1           the scalar tail's ``a0 +=`` (last block)
    2           (a0 + a1) + (a2 + a3)
    6           the xor butterfly over 64 lanes
    3           the four wave sums, added in wave order

so k = passes + 13.  The tests add the partials in float64, which adds nothing.  The ADAM
tail adds the nblk partials in index order (nblk - 1 more), takes ``sqrtf`` (which halves
the relative error and rounds once) and multiplies by grad_scale (one rounding)."""
import torch

from optim_reference import TINY, U, f32, make_vector, mlp_param_count  # noqa: F401

THREADS = 256
ARENA_32_64 = mlp_param_count(32, 64)       # 27,882 = 4 * 6970 + 2
ARENA_128_256 = mlp_param_count(128, 256)   # 136,074 = 4 * 34018 + 2
assert ARENA_32_64 == 27882 and ARENA_32_64 % 4 == 2 and ARENA_128_256 % 4 == 2
SIZES = (1, 2, 3, 4, 5, 1023, ARENA_32_64, ARENA_128_256)
NBLKS = (1, 7, 64)   # 64 > n / 4 for the six small sizes: empty slices
TAIL_MAG = 1.5       # |x| of the n % 4 tail elements of make_input


def slices(n: int, nblk: int):
    """[lo, hi) of every block, written out independently of ops.optim.clip_slices."""
    n4 = n // 4
    per = (n4 + nblk - 1) // nblk
    out = []
    for b in range(nblk):
        q0 = min(b * per, n4)
        q1 = min(q0 + per, n4)
        out.append((4 * q0, 4 * q1))
    lo, hi = out[-1]
    out[-1] = (lo if hi > lo else 4 * n4, n)   # the tail belongs to the last block
    return out


def partials_k(n: int, nblk: int) -> int:
    per = ((n // 4) + nblk - 1) // nblk
    passes = (per + THREADS - 1) // THREADS
    return passes + 13


def make_input(n: int, seed: int = 11) -> torch.Tensor:
    """Sign-mixed fp32 data of one scale; the scalar tail's elements have magnitude
    TAIL_MAG, so that losing them costs at least (n % 4) * 2.25 / sum(x^2) -- far beyond
    the bound at every size here (largest bound: n = 136,074, nblk = 1: 148 U = 8.8e-6
    relative, against a tail share of about 4.5 / 136,074 = 3.3e-5)."""
    x = make_vector(n, seed).clone()
    t = x[4 * (n // 4):]
    t.copy_(torch.where(t < 0, -TAIL_MAG, TAIL_MAG))
    return x


def ref_partials(x: torch.Tensor, nblk: int):
    """(float64 per-block sums of squares, float64 total, bound of the total)."""
    x = x.double().cpu().reshape(-1)
    part = torch.stack([(x[lo:hi] ** 2).sum() for lo, hi in slices(x.numel(), nblk)])
    s = float((x ** 2).sum())
    return part, s, (partials_k(x.numel(), nblk) + 1) * U * s + TINY


def norm_bound(n: int, nblk: int, norm: float) -> float:
    """|norm32 - norm64| allowed for sqrtf(sum of nblk partials) * grad_scale."""
    k_ss = partials_k(n, nblk) + nblk - 1
    return ((k_ss + 1) / 2 + 2 + 1) * U * abs(norm) + TINY


def coef_f32(max_norm: float, norm32: float) -> torch.Tensor:
    """min(1, max_norm / (norm + 1e-6)) evaluated in fp32 from an fp32 norm."""
    t = torch.tensor
    q = t(max_norm, dtype=torch.float32) / (t(norm32, dtype=torch.float32) + t(1e-6, dtype=torch.float32))
    return torch.minimum(t(1.0), q)


def ulps(a: float, b: float) -> int:
    """Distance of two finite fp32 values in units of the last place."""
    ia, ib = (int(torch.tensor(v, dtype=torch.float32).view(torch.int32)) for v in (a, b))
    return abs(ia - ib)
