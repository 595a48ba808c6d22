"""float64 stage references of the fused MNIST step (csrc/mlp_step3.hip) and of the forward
kernel ``mlp_eval`` (csrc/mlp_kernels.hip): the buffer-layout maps, the operand makers, the
a-priori rounding bounds and the exactness certificate that tests/test_mlp3_stages_fp64.py
holds the kernels to, element by element and stage by stage.  tests/test_mlp_reference.py
checks all of it on the CPU (against fp64 autograd, an fp32 / bf16 emulation of the kernels'
arithmetic and mutants of that emulation) before anything runs on a GPU.

Every stage is judged ALONE: its reference is computed in float64 from the kernel's own
output of the stage before (``xring`` -> ``h1pre`` -> H1 -> H2 -> dZ -> dH2 -> dH1 ->
gradients), so the chaotic propagation of bf16 roundings through the network, which forces
whole-tensor norm bounds on an end-to-end comparison, never enters.  Two instruments:

  * random operands under a bound computed from the reference alone.  U8 = 2^-8 is the bf16
    rounding of a stored result, U24 = 2^-24 the fp32 unit; a K-term fp32 sum in any order
    errs by at most K U24 A with A the same sum over absolute values, and the factor 2 covers
    the MFMA's internal adder (tests/test_conv_partition.py's accumulation term).  K is the
    reduction length the kernel really runs (L + 1 with the bias add, 16 for the class
    reduction of dH2, Bp for the gradients).  Layer 1 adds the 12.20 fixed point: 49 tile
    partials rounded to 2^-20 each, 49 2^-21 in all.  exp, log and the reciprocal of the
    softmax get a stated allowance of 2^-16 (about 256 fp32 ulps), not a measurement;
  * dyadic operands (pixels +-1, weights +-k/64 and +-k/16) for which ``exact_certificate``
    proves every fp32 partial sum in any order exact: the comparison is ``torch.equal``.

Buffer layouts (Bp = B rounded up to 32):
  h1pre [2 slots][copies][Bp L1] int32, 12.20 fixed point, MFMA-fragment order; copies add up
  xring [2][49][Bp][16] bf16      yring [2][Bp] int32 (-1 past the batch's rows)
  act   [L1 + 2 L2 + 16][Bp] bf16: rows H1T = 0, H2T = L1, DH2T = L1 + L2, DZT = L1 + 2 L2
  dh1t  [L1][Bp] bf16
Nothing here reads a kernel's output to decide a tolerance."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp

U8 = 2.0 ** -8
U24 = 2.0 ** -24
FIX = 2.0 ** 20           # h1pre's fixed point
SOFT = 2.0 ** -16         # allowance for __expf / __logf / the reciprocal of the softmax section
TILES = 49
NC = 10
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def _bf(t):
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------ layouts
def bp_of(B):
    return (int(B) + 31) // 32 * 32


def h1pre_pos(L1, Bp):
    """[Bp, L1] index of element (b, m) inside one h1pre copy."""
    b = torch.arange(Bp).view(-1, 1)
    m = torch.arange(L1).view(1, -1)
    return (((b // 16) * (L1 // 16) + m // 16) * 4 + b % 4) * 64 + ((b % 16) // 4) * 16 + m % 16


def h1pre_slots(h1pre, L1, Bp):
    """[2, Bp L1] int64: the copies of each ring slot summed (they add up)."""
    return h1pre.cpu().view(2, fused_mlp.mlp3_h1_copies(L1), Bp * L1).long().sum(1)


def h1pre_dense(slot_words, L1, Bp):
    """[Bp, L1] int64 fixed-point words of one (summed) slot; value = word / 2^20."""
    return slot_words.cpu().long()[h1pre_pos(L1, Bp)]


def h1pre_pack(dense, L1):
    """The inverse of h1pre_dense: [Bp, L1] words -> the flat slot."""
    Bp = dense.size(0)
    out = torch.zeros(Bp * L1, dtype=dense.dtype)
    out[h1pre_pos(L1, Bp).reshape(-1)] = dense.reshape(-1)
    return out


def xring_dense(xring, Bp):
    """[2, Bp, 784] float64 pixels of both ring slots."""
    return xring.cpu().view(2, TILES, Bp, 16).double().permute(0, 2, 1, 3).reshape(2, Bp, 784)


def xring_pack(dense):
    """[2, Bp, 784] -> the flat bf16 ring."""
    Bp = dense.size(1)
    return dense.view(2, Bp, TILES, 16).permute(0, 2, 1, 3).reshape(-1).to(torch.bfloat16)


def yring_dense(yring, Bp):
    return yring.cpu().view(2, Bp).long()


def act_rows(L1, L2):
    return {"H1T": 0, "H2T": L1, "DH2T": L1 + L2, "DZT": L1 + 2 * L2, "ROWS": L1 + 2 * L2 + 16}


def act_dense(act, dh1t, L1, L2, Bp):
    """The head's exported transposes as batch-major float64: h1 [Bp, L1], h2 [Bp, L2],
    dh2 [Bp, L2], dz [Bp, 16], dh1 [Bp, L1]."""
    r = act_rows(L1, L2)
    a = act.cpu().view(r["ROWS"], Bp).double()
    return {"h1": a[r["H1T"]:r["H2T"]].t().contiguous(), "h2": a[r["H2T"]:r["DH2T"]].t().contiguous(),
            "dh2": a[r["DH2T"]:r["DZT"]].t().contiguous(), "dz": a[r["DZT"]:r["ROWS"]].t().contiguous(),
            "dh1": dh1t.cpu().view(L1, Bp).double().t().contiguous()}


def act_pack(d, L1, L2):
    """The inverse of act_dense: (act, dh1t) flat bf16."""
    act = torch.cat([d["h1"].t(), d["h2"].t(), d["dh2"].t(), d["dz"].t()]).reshape(-1).to(torch.bfloat16)
    return act, d["dh1"].t().reshape(-1).to(torch.bfloat16)


Weights = namedtuple("Weights", "W1 b1 W2 b2 W3 b3 W2T W3T")


def weights_of(params, shadow, L1, L2):
    """What a head launch reads, as float64: the bf16 shadow's row-major W1 / W2 / W3 (layers
    1-3), its transposed W2^T [L1, L2] and W3^T [L2, 16] (dH1 / dH2) and the fp32 biases."""
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    sh = shadow.cpu().double()
    s = fused_mlp.mlp_unpack(sh[: lay["np"]], L1, L2)
    p = fused_mlp.mlp_unpack(params.cpu().double(), L1, L2)
    return Weights(s["layer_1.weight"], p["layer_1.bias"], s["layer_2.weight"], p["layer_2.bias"],
                   s["layer_3.weight"], p["layer_3.bias"], sh[lay["w2t"]:lay["w3t"]].view(L1, L2),
                   sh[lay["w3t"]:lay["total"]].view(L2, 16))


def shadow_invariants(params, shadow, L1, L2):
    """The shadow is bf16(params), its transposes are transposes (classes 10..15 zero)."""
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    w = weights_of(params, shadow, L1, L2)
    w3t = torch.zeros(L2, 16, dtype=torch.float64)
    w3t[:, :NC] = w.W3.t()
    return (torch.equal(shadow.cpu()[: lay["np"]], params.cpu().to(torch.bfloat16))
            and torch.equal(w.W2T, w.W2.t()) and torch.equal(w.W3T, w3t))


# ------------------------------------------------------------------ comparisons
Cmp = namedtuple("Cmp", "ok ratio detail")


def _first(bad):
    return bad.nonzero()[:4].tolist()


def cmp_equal(got, want) -> Cmp:
    """Value equality of every element (-0 == +0), shapes included."""
    if tuple(got.shape) != tuple(want.shape):
        return Cmp(False, float("inf"), f"shape {tuple(got.shape)} != {tuple(want.shape)}")
    g, w = got.double(), want.double()
    if torch.equal(g, w):
        return Cmp(True, 0.0, "equal")
    bad = g != w
    return Cmp(False, float("inf"), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {_first(bad)}, "
                                    f"largest by {float((g - w).abs().nan_to_num(float('inf')).max()):g}")


def cmp_bound(got, ref, bound) -> Cmp:
    """No element further than ``bound`` from ``ref`` (where the bound is 0: exactly equal).
    ratio = the worst error / bound."""
    if tuple(got.shape) != tuple(ref.shape):
        return Cmp(False, float("inf"), f"shape {tuple(got.shape)} != {tuple(ref.shape)}")
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return Cmp(False, float("inf"), "non-finite output")
    err = (g - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ratio > 1.0
    if not bool(bad.any()):
        return Cmp(True, worst, f"worst {worst:.3f}")
    return Cmp(False, worst, f"{int(bad.sum())} of {bad.numel()} elements past the bound, worst {worst:.3g}, "
                             f"first at {_first(bad)}")


def report(tag, results, worst=None):
    """Print the ``[bound ratio]`` line of a list of (stage, Cmp) and return the failures.
    ``worst``: a dict of running per-stage maxima to fold into."""
    line = " ".join(f"{s}={'exact' if c.ok and c.ratio == 0.0 else format(c.ratio, '.3f')}" for s, c in results)
    print(f"[bound ratio] {tag}: {line}")
    if worst is not None:
        for s, c in results:
            worst[s] = max(worst.get(s, 0.0), c.ratio)
    return [(s, c.detail) for s, c in results if not c.ok]


# ------------------------------------------------------------------ exactness
Cert = namedtuple("Cert", "ok granularity worst limit")


def granularity(t):
    """The largest power of two that divides every nonzero element (inf for all zeros)."""
    t = t.double().reshape(-1)
    t = t[t != 0]
    if t.numel() == 0:
        return float("inf")
    m, e = torch.frexp(t)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return float((low * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())).min())


def exact_certificate(a, w, bias=None) -> Cert:
    """a [M, K] and w [N, K] (bf16 or fp32 values held as doubles): with g the common binary
    granularity of all products (and the bias), ``sum_k |a||w| (+ |bias|) < 2^24 g`` for every
    output means every partial sum of a . w^T (+ bias), in any order and grouping, is an
    integer multiple of g below 2^24 g, hence an fp32 number: the GEMM is exact on the MFMA
    and anywhere else."""
    a, w = a.double(), w.double()
    g = granularity(a) * granularity(w)
    amp = a.abs() @ w.abs().t()
    if bias is not None:
        g = min(g, granularity(bias))
        amp = amp + bias.double().abs()
    if g == float("inf"):  # an all-zero operand
        return Cert(True, g, 0.0, g)
    worst = float(amp.max())
    return Cert(worst < 2.0 ** 24 * g, g, worst, 2.0 ** 24 * g)


# ------------------------------------------------------------------ operands
def random_data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def random_params(L1, L2, seed):
    return fused_mlp.init_mlp_params(L1, L2, torch.Generator().manual_seed(seed))


NORM_PM1 = ((0.5,), (0.5,))   # Normalize under which the bytes {0, 255} are exactly -1.0 / +1.0


def exact_data(n, seed, family="nozero"):
    """``nozero``: bytes {0, 255} (with NORM_PM1: pixels -1 / +1, no zeros anywhere);
    ``prod``: bytes in [128, 255] under the default map: bf16(u8 / 255) in [0.5, 1] is a multiple
    of 2^-8, so layer 1's products are multiples of 2^-14 and layer 2's of 2^-20."""
    g = torch.Generator().manual_seed(seed)
    if family == "nozero":
        x = (torch.randint(0, 2, (n, 784), generator=g) * 255).to(torch.uint8)
    else:
        x = torch.randint(128, 256, (n, 784), generator=g, dtype=torch.uint8)
    return x, torch.randint(0, 10, (n,), generator=g)


def exact_params(L1, L2, seed):
    """W1, b1, W2, b2 = +-k/64 (k in 1..8), W3, b3 = +-k/16 (k in 1..4): a flat fp32 arena."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.empty(fused_mlp.mlp_param_count(L1, L2))
    for name, t in fused_mlp.mlp_unpack(flat, L1, L2).items():
        kmax, den = (4, 16.0) if name.startswith("layer_3") else (8, 64.0)
        mag = torch.randint(1, kmax + 1, t.shape, generator=g)
        sign = torch.randint(0, 2, t.shape, generator=g) * 2 - 1
        t.copy_((mag * sign).float() / den)
    return flat


def int_plant(shape, seed):
    """Integers in {+-1, .., +-4}, no zeros (exact in bf16)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(1, 5, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).double()


# ------------------------------------------------------------------ stage references
def ref_gather(x_u8, labels, idx, Bp, x_scale=fused_mlp.X_SCALE_DEFAULT, x_shift=0.0):
    """(X [Bp, 784] float64 of bf16 values, y [Bp]) of the batch ``idx``: rows past it are zero
    pixels with label -1."""
    rows = idx.numel()
    X = torch.zeros(Bp, 784, dtype=torch.float64)
    X[:rows] = _bf(fused_mlp.u8_to_input(x_u8[idx], x_scale, x_shift))
    y = torch.full((Bp,), -1, dtype=torch.long)
    y[:rows] = labels[idx]
    return X, y


def ref_layer1(X, W1):
    """(X . W1^T, bound): 49 tile partials of 16 pixels (MFMA, fp32), each rounded to 2^-20
    (half a unit of error apiece), added as integers.  Tile partials beyond +-32 would be
    clamped; the reference refuses operands that reach them."""
    xt, wt = X.view(X.size(0), TILES, 16), W1.view(W1.size(0), TILES, 16)
    amp_t = torch.einsum("bti,mti->tbm", xt.abs(), wt.abs())
    assert float(amp_t.max()) < 32.0, "a layer-1 tile partial can reach the 12.20 clamp"
    return X @ W1.t(), TILES * 2.0 ** -21 + (2.0 * 16 * U24 * amp_t).sum(0)


def layer1_exact_q(X, W1):
    """int64 sum of x w 2^20 (operands for which every tile partial is exact and a multiple of 2^-20)."""
    q = (X @ W1.t()) * FIX
    assert torch.equal(q, q.round()), "layer 1 is not exact in 12.20 for these operands"
    return q.to(torch.int64)


def ref_h1(q, b1):
    """The kernel's own operations on the fixed-point words: bf16(relu(float32(q) 2^-20 + b1)),
    every step in fp32, one rounding each (fixed_to_f32, relu_bf)."""
    h = q.to(torch.float32) * (1.0 / 1048576.0) + b1.to(torch.float32)
    return torch.relu(h).to(torch.bfloat16).double()


def _linear(a, w, bias=None):
    ref, amp = a @ w.t(), a.abs() @ w.abs().t()
    if bias is not None:
        ref, amp = ref + bias, amp + bias.abs()
    return ref, amp


def ref_h2(H1, W2, b2):
    ref, amp = _linear(H1, W2, b2)
    ref = torch.relu(ref)
    return ref, U8 * ref + 2.0 * (W2.size(1) + 1) * U24 * amp


def ref_logits(H2, W3, b3):
    """(Z [rows, 10], ez): the logits are not exported; ez bounds the kernel's own."""
    ref, amp = _linear(H2, W3, b3)
    return ref, 2.0 * (W3.size(1) + 1) * U24 * amp


def ref_dz(Z, ez, y, rows):
    """((softmax(Z) - onehot) / rows as [n, 16], bound): rows with label -1 and class slots
    10..15 are exactly zero (bound 0).  t = (max_j ez / 2 + 2^-16) / rows: a softmax moves by at
    most half the largest logit error; U8 is the bf16 store."""
    n = Z.size(0)
    ok = (y >= 0).view(-1, 1)
    d = torch.softmax(Z, 1) - F.one_hot(y.clamp_min(0), NC).double()
    t = (ez.max(1, keepdim=True).values / 2.0 + SOFT) / rows
    ref, bound = torch.zeros(n, 16, dtype=torch.float64), torch.zeros(n, 16, dtype=torch.float64)
    ref[:, :NC] = torch.where(ok, d / rows, torch.zeros_like(d))
    bound[:, :NC] = torch.where(ok, U8 * (ref[:, :NC].abs() + t) + t, torch.zeros_like(d))
    return ref, bound


Stats = namedtuple("Stats", "loss loss_bound certain ambiguous rows")


def ref_stats(Z, ez, y):
    """The stats row of the rows with a label: mean NLL and its bound
    mean_r(2 max_j ez + 2^-16 (|m| + |lse| + |z_y|)); the rows whose two largest logits lie
    within 2 max ez of each other are ambiguous, the others certainly right or wrong (a tie
    goes to the lowest class)."""
    v = y >= 0
    Zv, ev, yv = Z[v], ez[v], y[v]
    m = Zv.max(1).values
    lse = m + torch.log(torch.exp(Zv - m.view(-1, 1)).sum(1))
    zy = Zv.gather(1, yv.view(-1, 1)).squeeze(1)
    emax = ev.max(1).values
    loss = float((lse - zy).mean())
    bound = float((2.0 * emax + SOFT * (m.abs() + lse.abs() + zy.abs())).mean())
    top = Zv.topk(2, dim=1).values
    amb = (top[:, 0] - top[:, 1]) < 2.0 * emax
    pred = torch.where(Zv == m.view(-1, 1), torch.arange(NC).expand_as(Zv), torch.full_like(Zv, NC, dtype=torch.long)
                       ).min(1).values
    return Stats(loss, bound, int(((pred == yv) & ~amb).sum()), int(amb.sum()), int(v.sum()))


def ref_dh2(dZ, W3T, H2):
    """(dZ W3) masked by the kernel's own H2 > 0; one 32-deep MFMA over 16 class slots."""
    ref, amp = dZ @ W3T.t(), dZ.abs() @ W3T.abs().t()
    mask = (H2 > 0).double()
    ref = ref * mask
    return ref, U8 * ref.abs() + 2.0 * 16 * U24 * amp * mask


def ref_dh1(dH2, W2T, H1):
    ref, amp = dH2 @ W2T.t(), dH2.abs() @ W2T.abs().t()
    mask = (H1 > 0).double()
    ref = ref * mask
    return ref, U8 * ref.abs() + 2.0 * W2T.size(1) * U24 * amp * mask


def ref_grads(obs):
    """{name: (ref, amp)} of the six gradients from the tail's own operands over all Bp batch
    columns: dW1 = dH1^T X, dW2 = dH2^T H1, dW3 = dZ^T H2 (classes 0..9), db = row sums."""
    def mm(d, a):
        return d.t() @ a, d.abs().t() @ a.abs()

    dz = obs["dz"][:, :NC]
    out = {"W1": mm(obs["dh1"], obs["x"]), "W2": mm(obs["dh2"], obs["h1"]), "W3": mm(dz, obs["h2"])}
    for k, d in (("b1", obs["dh1"]), ("b2", obs["dh2"]), ("b3", dz)):
        out[k] = (d.sum(0), d.abs().sum(0))
    return out


def flat_grads(refs):
    return torch.cat([refs[k][0].reshape(-1) for k in NAMES]), torch.cat([refs[k][1].reshape(-1) for k in NAMES])


def grad_checks(g, obs, L1, L2, exact=False):
    """[(name, Cmp)] of a flat fp32 gradient against ref_grads(obs): within 2 Bp U24 amp per
    element (no bf16 term: the output is fp32; amp = 0 demands an exact zero), or -- planted
    integer operands -- equal."""
    Bp = obs["x"].size(0)
    refs = ref_grads(obs)
    got = fused_mlp.mlp_unpack(g.cpu().double(), L1, L2)
    out = []
    for k, t in zip(NAMES, got.values()):
        ref, amp = refs[k]
        out.append(("d" + k, cmp_equal(t, ref) if exact else cmp_bound(t, ref, 2.0 * Bp * U24 * amp)))
    return out


# ------------------------------------------------------------------ the head, stage by stage
def head_checks(obs, wt, rows, step, exact=False, exact_through_h2=False, handoff_only=False):
    """[(stage, Cmp)] of one head pass.  ``obs``: what the launch read and wrote, batch-major
    float64 over all Bp rows -- x, y (the consumed ring slot), q / q_other (the consumed and the
    other h1pre slot before the step, int64 words), h1, h2, dz, dh2, dh1 (act_dense), stats
    (the step's row) -- and x_want / y_want (ref_gather of the batch that should be there).
    ``rows``: the batch's valid rows.  ``exact``: the dyadic no-zeros family (every GEMM of the
    forward pass certified exact, so ez = 0); ``exact_through_h2``: certified through H2, and
    layer 3 (ez = 0) where its own certificate passes.  ``handoff_only``: the buffers handed from
    launch to launch alone (gather, labels, layer1, other_slot) -- what a route that exports no
    act / dh1t still leaves to check."""
    out = []
    X, y = obs["x"], obs["y"]
    out.append(("gather", cmp_equal(X, obs["x_want"])))
    out.append(("labels", cmp_equal(y, obs["y_want"])))
    pad = torch.arange(X.size(0)) >= rows
    q = obs["q"]
    # layer 1: padded rows and the other slot exactly zero
    if exact or exact_through_h2:
        out.append(("layer1", cmp_equal(q, layer1_exact_q(X, wt.W1))))
    else:
        ref, bound = ref_layer1(X, wt.W1)
        bound = torch.where(pad.view(-1, 1), torch.zeros_like(bound), bound)
        out.append(("layer1", cmp_bound(q.double() / FIX, ref, bound)))
    out.append(("other_slot", cmp_equal(obs["q_other"], torch.zeros_like(obs["q_other"]))))
    if handoff_only:
        return out
    out.append(("H1", cmp_equal(obs["h1"], ref_h1(q, wt.b1))))
    H1, H2 = obs["h1"], obs["h2"]
    ref, bound = ref_h2(H1, wt.W2, wt.b2)
    if exact or exact_through_h2:
        c = exact_certificate(H1, wt.W2, wt.b2)
        out.append(("H2", cmp_equal(H2, _bf(ref)) if c.ok else Cmp(False, float("inf"), f"layer 2 not certified: {c}")))
    else:
        out.append(("H2", cmp_bound(H2, ref, bound)))
    Z, ez = ref_logits(H2, wt.W3, wt.b3)
    if exact or exact_through_h2:
        c = exact_certificate(H2, wt.W3, wt.b3)
        if c.ok:  # the operands' verdict, never the output's
            ez = torch.zeros_like(ez)
        elif exact:
            out.append(("certificate", Cmp(False, float("inf"), f"layer 3 not certified: {c}")))
    ref, bound = ref_dz(Z, ez, y, rows)
    out.append(("dZ", cmp_bound(obs["dz"], ref, bound)))
    st = ref_stats(Z, ez, y)
    got = obs["stats"].double()
    out.append(("loss", cmp_bound(got[0:1], torch.tensor([st.loss], dtype=torch.float64), st.loss_bound)))
    # the count lies in [certain, certain + ambiguous]; nothing is ambiguous with exact logits, nor at
    # the committed initial weights (tests/test_mlp_reference.py), so this is equality nearly everywhere
    lo = torch.tensor([st.certain, rows, step], dtype=torch.float64)
    hi = torch.tensor([st.certain + st.ambiguous, rows, step], dtype=torch.float64)
    ok = bool(((got[1:] >= lo) & (got[1:] <= hi)).all())
    out.append(("count", Cmp(ok, 0.0 if ok else float("inf"),
                             "equal" if ok else f"(correct, rows, step) {got[1:].tolist()} outside {lo.tolist()} .. "
                                                f"{hi.tolist()}")))
    ref, bound = ref_dh2(obs["dz"], wt.W3T, H2)
    out.append(("dH2", cmp_bound(obs["dh2"], ref, bound)))
    ref, bound = ref_dh1(obs["dh2"], wt.W2T, H1)
    out.append(("dH1", cmp_bound(obs["dh1"], ref, bound)))
    return out


# ------------------------------------------------------------------ the whole chain, no rounding
def chain_fp64(p, X, y):
    """The stage functions composed without any rounding: (loss, {name: gradient}) in float64,
    what fp64 autograd gives (tests/test_mlp_reference.py).  ``p``: the six tensors, float64."""
    W1, b1, W2, b2, W3, b3 = p
    rows = X.size(0)
    H1 = torch.relu(X @ W1.t() + b1)
    H2, _ = ref_h2(H1, W2, b2)
    Z, ez = ref_logits(H2, W3, b3)
    dz, _ = ref_dz(Z, ez, y, rows)
    w3t = torch.zeros(W3.size(1), 16, dtype=torch.float64)
    w3t[:, :NC] = W3.t()
    dh2, _ = ref_dh2(dz, w3t, H2)
    dh1, _ = ref_dh1(dh2, W2.t().contiguous(), H1)
    g = ref_grads({"x": X, "h1": H1, "h2": H2, "dz": dz, "dh2": dh2, "dh1": dh1})
    return ref_stats(Z, ez, y).loss, {k: v[0] for k, v in g.items()}


# ------------------------------------------------------------------ fp32 / bf16 emulation
def emulate_head(X, y, wt, rows, step, trunc=False):
    """The kernels' arithmetic in torch fp32 / bf16 (sums in index order, an fp32 softmax):
    an ``obs`` for head_checks, every stage fed by the emulation's own stage before.  ``trunc``:
    store bf16 by truncation instead of round-to-nearest (a mutant)."""
    def bf(t):
        t = t.float()
        if trunc:
            return (t.view(torch.int32) & -65536).view(torch.float32).double()
        return t.to(torch.bfloat16).double()

    f = torch.float32
    Bp = X.size(0)
    part = torch.einsum("bti,mti->tbm", X.view(Bp, TILES, 16).to(f), wt.W1.view(-1, TILES, 16).to(f))
    q = torch.round(part.double() * FIX).clamp(-2.0 ** 25, 2.0 ** 25).to(torch.int64).sum(0)
    h1 = bf(torch.relu(q.to(f) * (1.0 / 1048576.0) + wt.b1.to(f)))
    h2 = bf(torch.relu(h1.to(f) @ wt.W2.to(f).t() + wt.b2.to(f)))
    z = h2.to(f) @ wt.W3.to(f).t() + wt.b3.to(f)
    m = z.max(1, keepdim=True).values
    p = torch.exp(z - m)
    s = p.sum(1, keepdim=True)
    ok = (y >= 0).view(-1, 1)
    invB = torch.tensor(1.0, dtype=f) / torch.tensor(float(rows), dtype=f)
    d = (p * (1.0 / s) - F.one_hot(y.clamp_min(0), NC).to(f)) * invB
    dz = torch.zeros(Bp, 16, dtype=torch.float64)
    dz[:, :NC] = torch.where(ok, bf(d), torch.zeros(Bp, NC, dtype=torch.float64))
    nll = torch.where(ok.squeeze(1), (m + torch.log(s)).squeeze(1) - z.gather(1, y.clamp_min(0).view(-1, 1)).squeeze(1),
                      torch.zeros(Bp, dtype=f))
    hit = ((z.argmax(1) == y) & ok.squeeze(1)).sum()
    stats = torch.tensor([float(nll.sum() * invB), float(hit), float(ok.sum()), float(step)])
    dh2 = torch.where(h2 > 0, bf(dz.to(f) @ wt.W3T.to(f).t()), torch.zeros_like(h2))
    dh1 = torch.where(h1 > 0, bf(dh2.to(f) @ wt.W2T.to(f).t()), torch.zeros_like(h1))
    return {"x": X, "y": y, "q": q, "q_other": torch.zeros_like(q), "h1": h1, "h2": h2, "dz": dz, "dh2": dh2,
            "dh1": dh1, "stats": stats, "x_want": X.clone(), "y_want": y.clone()}


def emulate_grads(obs):
    """The tail's fp32 gradients of an ``obs`` (flat, arena order)."""
    f = torch.float32
    dz = obs["dz"][:, :NC].to(f)
    x, h1, h2, dh2, dh1 = (obs[k].to(f) for k in ("x", "h1", "h2", "dh2", "dh1"))
    g = [dh1.t() @ x, dh1.sum(0), dh2.t() @ h1, dh2.sum(0), dz.t() @ h2, dz.sum(0)]
    return torch.cat([t.reshape(-1) for t in g])
