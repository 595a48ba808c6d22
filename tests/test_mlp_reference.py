"""tests/mlp_reference.py checked on the CPU, before anything runs on a GPU: the fp64 stage
chain against fp64 autograd, an fp32 / bf16 emulation of the kernels' arithmetic inside every
bound (worst ratios printed), mutants of that emulation outside them, the exactness
certificate on the committed dyadic operands of every engine and mlp_eval case of the GPU file
(and its refusal of default-init weights), zero ambiguous rows for every committed (seed,
shape), and the layout maps' round trips."""
import pytest
import torch
import torch.nn.functional as F

import mlp_reference as R
from ray_lightning_accelerators_amd.ops import fused_mlp

# (L1, L2, B, rows): the shapes the feasibility of the bounds was worked out at, a short batch,
# and the widest pair at several head blocks
EMU_CASES = [(32, 64, 32, 32), (128, 256, 100, 100), (64, 128, 17, 17), (32, 64, 32, 24), (64, 128, 64, 33),
             (128, 256, 256, 256), (32, 32, 1, 1)]


def _weights(params, L1, L2):
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    shadow = torch.zeros(lay["total"], dtype=torch.bfloat16)
    fused_mlp.mlp_refresh_shadow(params, shadow, L1, L2)
    assert R.shadow_invariants(params, shadow, L1, L2)
    return R.weights_of(params, shadow, L1, L2)


def _random_case(L1, L2, B, rows, seed=None):
    seed = L1 + L2 + B + rows if seed is None else seed
    x, y = R.random_data(B + 3, seed)
    idx = torch.randperm(B + 3, generator=torch.Generator().manual_seed(seed))[:rows]
    X, yb = R.ref_gather(x, y, idx, R.bp_of(B))
    return X, yb, _weights(R.random_params(L1, L2, seed), L1, L2)


def _exact_case(L1, L2, B, rows, family="nozero", seed=None):
    seed = L1 + L2 + B + rows if seed is None else seed
    x, y = R.exact_data(B + 3, seed, family)
    idx = torch.randperm(B + 3, generator=torch.Generator().manual_seed(seed))[:rows]
    aff = fused_mlp.input_affine(R.NORM_PM1) if family == "nozero" else fused_mlp.input_affine(None)
    X, yb = R.ref_gather(x, y, idx, R.bp_of(B), *aff)
    return X, yb, _weights(R.exact_params(L1, L2, seed), L1, L2)


def test_chain_without_rounding_is_fp64_autograd():
    for L1, L2, rows in ((32, 64, 24), (64, 128, 17), (128, 256, 40)):
        g = torch.Generator().manual_seed(L1 + rows)
        p = [t.double().requires_grad_(True) for t in fused_mlp.mlp_unpack(R.random_params(L1, L2, 5), L1, L2).values()]
        X = torch.rand(rows, 784, generator=g, dtype=torch.float64)
        y = torch.randint(0, 10, (rows,), generator=g)
        h = torch.relu(F.linear(torch.relu(F.linear(X, p[0], p[1])), p[2], p[3]))
        loss = F.nll_loss(F.log_softmax(F.linear(h, p[4], p[5]), 1), y)
        grads = torch.autograd.grad(loss, p)
        got_loss, got = R.chain_fp64([t.detach() for t in p], X, y)
        assert abs(got_loss - float(loss.detach())) < 1e-12
        for k, ref in zip(R.NAMES, grads):
            assert float((got[k] - ref).abs().max()) < 1e-12, k


@pytest.mark.parametrize("L1,L2,B,rows", EMU_CASES)
def test_emulation_stays_inside_every_bound(L1, L2, B, rows):
    X, y, wt = _random_case(L1, L2, B, rows)
    obs = R.emulate_head(X, y, wt, rows, 3)
    res = R.head_checks(obs, wt, rows, 3) + R.grad_checks(R.emulate_grads(obs), obs, L1, L2)
    bad = R.report(f"emulation {L1}/{L2} B={B} rows={rows}", res)
    assert not bad, bad


@pytest.mark.parametrize("L1,L2,B,rows", [(32, 64, 32, 32), (64, 128, 17, 17), (128, 256, 100, 100),
                                          (128, 256, 64, 64), (64, 128, 64, 7)])
def test_exact_family_is_certified_and_the_emulation_reproduces_it(L1, L2, B, rows):
    """No-zeros family: every forward GEMM certified, so H1 / H2 are ``torch.equal`` and an fp32
    matmul reproduces the fp64 logits bitwise; no row's two largest logits tie (with exact logits
    any gap, one unit of their 2^-16 grid included, is decided the same way everywhere)."""
    X, y, wt = _exact_case(L1, L2, B, rows)
    assert float(X[:rows].abs().min()) == 1.0 and float(X[:rows].abs().max()) == 1.0  # -1 / +1, no zeros
    obs = R.emulate_head(X, y, wt, rows, 2)
    res = R.head_checks(obs, wt, rows, 2, exact=True) + R.grad_checks(R.emulate_grads(obs), obs, L1, L2)
    bad = R.report(f"exact {L1}/{L2} B={B} rows={rows}", res)
    assert not bad, bad
    c2, c3 = R.exact_certificate(obs["h1"], wt.W2, wt.b2), R.exact_certificate(obs["h2"], wt.W3, wt.b3)
    print(f"[certificate] {L1}/{L2}: layer 2 {c2.worst / c2.limit:.3f}, layer 3 {c3.worst / c3.limit:.3f} of the limit")
    assert c2.ok and c3.ok and c3.worst * 4 <= c3.limit and c2.worst * 4 <= c2.limit  # with room to spare
    Z, _ = R.ref_logits(obs["h2"][:rows], wt.W3, wt.b3)
    z32 = obs["h2"][:rows].float() @ wt.W3.float().t() + wt.b3.float()
    assert torch.equal(z32.double(), Z)
    top = Z.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 0.0


@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 64), (128, 256, 100)])
def test_production_map_family_is_certified_through_h2_only(L1, L2, B):
    X, y, wt = _exact_case(L1, L2, B, B, family="prod")
    obs = R.emulate_head(X, y, wt, B, 2)
    xt, wv = X.view(-1, R.TILES, 16), wt.W1.view(-1, R.TILES, 16)
    for t in (0, 17, 48):  # layer 1, per 16-pixel tile
        assert R.exact_certificate(xt[:, t], wv[:, t]).ok
    assert R.granularity(X) * R.granularity(wt.W1) >= 2.0 ** -20  # and every partial is a 12.20 word
    c2, c3 = R.exact_certificate(obs["h1"], wt.W2, wt.b2), R.exact_certificate(obs["h2"], wt.W3, wt.b3)
    print(f"[certificate] prod {L1}/{L2}: layer 2 {c2.worst / c2.limit:.3f}, layer 3 {c3.worst / c3.limit:.3f}")
    assert c2.ok and (L2 < 256 or not c3.ok)  # the widest layer 3 is past the certificate: bounded instead
    bad = R.report(f"prod {L1}/{L2} B={B}", R.head_checks(obs, wt, B, 2, exact_through_h2=True))
    assert not bad, bad


def test_certificate_refuses_default_init_weights():
    X, y, wt = _random_case(32, 64, 32, 32)
    obs = R.emulate_head(X, y, wt, 32, 1)
    assert not R.exact_certificate(obs["h1"], wt.W2, wt.b2).ok
    assert not R.exact_certificate(obs["h2"], wt.W3, wt.b3).ok
    # and the arithmetic it certifies: 2^24 + 1 is the first integer fp32 cannot hold
    a = torch.ones(1, 2, dtype=torch.float64)
    assert R.exact_certificate(a, torch.tensor([[2.0 ** 23, 2.0 ** 23 - 1]], dtype=torch.float64)).ok
    assert not R.exact_certificate(a, torch.tensor([[2.0 ** 24, 1.0]], dtype=torch.float64)).ok
    assert R.granularity(torch.tensor([0.75, 0.0, 6.0])) == 0.25


# ------------------------------------------------------------------ mutants
def _fails(obs, wt, rows, L1, L2, g=None, exact=False):
    g = R.emulate_grads(obs) if g is None else g
    res = R.head_checks(obs, wt, rows, 3, exact=exact) + R.grad_checks(g, obs, L1, L2)
    return [s for s, c in res if not c.ok]


@pytest.mark.parametrize("L1,L2,B,rows", [(32, 64, 32, 32), (128, 256, 100, 100), (64, 128, 32, 17)])
def test_mutants_of_the_emulation_are_caught(L1, L2, B, rows):
    X, y, wt = _random_case(L1, L2, B, rows)
    f = torch.float32

    def fresh():
        return {k: v.clone() for k, v in R.emulate_head(X, y, wt, rows, 3).items()}

    assert _fails(fresh(), wt, rows, L1, L2) == []
    # one dropped batch row of dW1
    o = fresh()
    o2 = dict(o, dh1=o["dh1"].clone())
    o2["dh1"][rows - 1] = 0
    g = R.emulate_grads(o2)
    assert "dW1" in _fails(o, wt, rows, L1, L2, g=g)
    # one dropped k-term of layer 2
    o = fresh()
    keep = torch.arange(L1) != int(o["h1"].abs().sum(0).argmax())  # a live unit's term
    o["h2"] = torch.relu(o["h1"][:, keep].to(f) @ wt.W2[:, keep].to(f).t() + wt.b2.to(f)).to(torch.bfloat16).double()
    assert "H2" in _fails(o, wt, rows, L1, L2)
    # two swapped columns of one 16x16 tile of dW1
    o = fresh()
    n1 = L1 * 784
    g = R.emulate_grads(o)
    w1 = g[:n1].view(L1, 784)
    w1[16:32, [162, 165]] = w1[16:32, [165, 162]]
    assert "dW1" in _fails(o, wt, rows, L1, L2, g=g)
    # a swapped pair of columns of H2
    o = fresh()
    o["h2"][:, [3, 4]] = o["h2"][:, [4, 3]]
    assert "H2" in _fails(o, wt, rows, L1, L2)
    # a nonzero padded column
    if rows < R.bp_of(B):
        for k in ("dz", "dh2", "dh1"):
            o = fresh()
            o[k][rows, 0] = 2.0 ** -10
            assert {"dz": "dZ", "dh2": "dH2", "dh1": "dH1"}[k] in _fails(o, wt, rows, L1, L2)
        o = fresh()
        o["q"][rows, 1] = 1
        assert "layer1" in _fails(o, wt, rows, L1, L2)
    # a label taken from the neighbouring row
    o = fresh()
    o["y"][:rows] = o["y"][:rows].roll(1)
    assert "labels" in _fails(o, wt, rows, L1, L2)
    if rows > 1:
        o = R.emulate_head(X, torch.cat([y[:rows].roll(1), y[rows:]]), wt, rows, 3)
        o["y"], o["y_want"] = y.clone(), y.clone()
        assert "dZ" in _fails(o, wt, rows, L1, L2)
    # bf16 truncation instead of round-to-nearest
    o = {k: v.clone() for k, v in R.emulate_head(X, y, wt, rows, 3, trunc=True).items()}
    bad = _fails(o, wt, rows, L1, L2)
    assert "H1" in bad and "H2" in bad
    # the other h1pre slot not zeroed
    o = fresh()
    o["q_other"][0, 0] = 1
    assert "other_slot" in _fails(o, wt, rows, L1, L2)
    # H1 one bf16 step off in one element
    o = fresh()
    live = (o["h1"][0] > 0).nonzero()[0, 0]
    o["h1"][0, live] *= 1.0 + 2.0 ** -7
    assert "H1" in _fails(o, wt, rows, L1, L2)
    # a wrong count, a wrong row count, a wrong step in the stats row
    for col in (1, 2, 3):
        o = fresh()
        o["stats"][col] += 1
        assert "count" in _fails(o, wt, rows, L1, L2)


def test_mutant_one_over_b_on_a_short_batch():
    L1, L2, B, rows = 32, 64, 32, 24
    X, y, wt = _random_case(L1, L2, B, rows)
    o = R.emulate_head(X, y, wt, B, 3)       # scaled by 1 / B
    o["stats"][2] = rows
    bad = _fails(o, wt, rows, L1, L2)
    assert "dZ" in bad and "loss" in bad


def test_mutants_of_the_exact_family():
    L1, L2, B, rows = 32, 64, 32, 32
    X, y, wt = _exact_case(L1, L2, B, rows)
    o = R.emulate_head(X, y, wt, rows, 3)
    assert _fails(o, wt, rows, L1, L2, exact=True) == []
    o["q"][5, 7] += 1                         # one 2^-20 unit in one layer-1 sum
    assert "layer1" in _fails(o, wt, rows, L1, L2, exact=True)
    o = R.emulate_head(X, y, wt, rows, 3)
    o["h2"][3, 9] += 2.0 ** -12               # one unit of the layer-2 grid
    assert "H2" in _fails(o, wt, rows, L1, L2, exact=True)
    # planted integers: one dropped row changes every element it touches
    obs = {"x": R.int_plant((32, 784), 1), "h1": R.int_plant((32, L1), 2), "h2": R.int_plant((32, L2), 3),
           "dh2": R.int_plant((32, L2), 4), "dh1": R.int_plant((32, L1), 5), "dz": R.int_plant((32, 16), 6)}
    g = R.emulate_grads(obs)
    assert all(c.ok for _, c in R.grad_checks(g, obs, L1, L2, exact=True))
    o2 = dict(obs, dh2=obs["dh2"].clone())
    o2["dh2"][31] = 0
    bad = [s for s, c in R.grad_checks(R.emulate_grads(o2), obs, L1, L2, exact=True) if not c.ok]
    assert bad == ["dW2", "db2"]


# ------------------------------------------------------------------ committed seeds: no ambiguous row
def test_committed_cases_are_certified_and_have_no_ambiguous_row():
    """Every sample of every committed dataset at the committed initial weights, before anything
    runs on a GPU.  Dyadic families: layer 1 is exact in 12.20 (``layer1_exact_q``, and no tile
    partial near the clamp), layer 2 passes the certificate, layer 3 too in the no-zeros family
    (the production map: by its verdict); their lr is 0, so these are the weights of every step.
    No row's two largest logits lie within 2 max ez of each other (dyadic: no tie).  A
    random-family engine moves its weights; its own steps hold the count to the interval."""
    import test_mlp3_stages_fp64 as G

    for L1, L2, B, family, world in G.committed_cases():
        x, y, params, norm, _ = G.make_case(L1, L2, B, family, world)
        n = x.size(0)
        assert n // world // B == G.NB or B == 1   # set_data makes NB batches per epoch and rank
        X, yb = R.ref_gather(x, y, torch.arange(n), n, *fused_mlp.input_affine(norm))
        wt = _weights(params, L1, L2)
        obs = R.emulate_head(X, yb, wt, n, 1)
        Z, ez = R.ref_logits(obs["h2"], wt.W3, wt.b3)
        if family != "random":
            assert torch.equal(R.layer1_exact_q(X, wt.W1), obs["q"]), (L1, L2, B, family)
            assert R.exact_certificate(obs["h1"], wt.W2, wt.b2).ok, (L1, L2, B, family)
            if R.exact_certificate(obs["h2"], wt.W3, wt.b3).ok:
                ez = torch.zeros_like(ez)
            else:
                assert family == "prod", (L1, L2, B, family)
        st = R.ref_stats(Z, ez, yb)
        assert st.ambiguous == 0 and st.rows == n, (L1, L2, B, family, world, st)


def test_committed_mlp_eval_operands_are_certified():
    """The operands of every mlp_eval case of the GPU file: all three GEMMs certified exact (the
    production map: layers 1 and 2), no tie between a row's two largest logits."""
    import test_mlp3_stages_fp64 as G

    cases = [(L1, L2, n, mode, "nozero") for L1, L2 in G.EVAL_WIDTHS for n in G.EVAL_N for mode in ("u8", "f32")]
    cases += [(L1, L2, n, "u8", "prod") for L1, L2, n in G.EVAL_PROD]
    for L1, L2, n, mode, family in cases:
        params, X, yb = G.eval_operands(L1, L2, n, mode, family)[:3]
        W1, b1, W2, b2, W3, b3 = fused_mlp.mlp_unpack(params.double(), L1, L2).values()
        assert torch.equal(params.to(torch.bfloat16).float(), params)   # the weights are bf16 numbers
        assert R.exact_certificate(X, W1, b1).ok, (L1, L2, n, mode, family)
        H1 = torch.relu(X @ W1.t() + b1).to(torch.bfloat16).double()
        assert R.exact_certificate(H1, W2, b2).ok, (L1, L2, n, mode, family)
        H2 = torch.relu(H1 @ W2.t() + b2).to(torch.bfloat16).double()
        c3 = R.exact_certificate(H2, W3, b3)
        assert c3.ok or family == "prod", (L1, L2, n, mode, family, c3)
        Z, ez = R.ref_logits(H2, W3, b3)
        assert R.ref_stats(Z, torch.zeros_like(ez) if c3.ok else ez, yb).ambiguous == 0, (L1, L2, n, mode, family)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("L1,Bp", [(32, 32), (64, 64), (128, 256), (32, 96)])
def test_layout_maps_round_trip(L1, Bp):
    L2 = 64
    g = torch.Generator().manual_seed(L1 + Bp)
    pos = R.h1pre_pos(L1, Bp).reshape(-1)
    assert torch.equal(pos.sort().values, torch.arange(Bp * L1))          # a permutation of the slot
    dense = torch.randint(-2 ** 25, 2 ** 25, (Bp, L1), generator=g)
    assert torch.equal(R.h1pre_dense(R.h1pre_pack(dense, L1), L1, Bp), dense)
    # a head block's 32 rows are one contiguous range of the slot (what the kernels zero and load)
    blk = R.h1pre_pos(L1, Bp)[32 * (Bp // 32 - 1):].reshape(-1)
    assert int(blk.min()) == (Bp - 32) * L1 and int(blk.max()) == Bp * L1 - 1
    copies = fused_mlp.mlp3_h1_copies(L1)
    raw = torch.randint(-1000, 1000, (2 * copies * Bp * L1,), generator=g, dtype=torch.int32)
    assert torch.equal(R.h1pre_slots(raw, L1, Bp), raw.view(2, copies, -1).long().sum(1))
    x = torch.randn(2, Bp, 784, generator=g).to(torch.bfloat16).double()
    ring = R.xring_pack(x)
    assert ring.numel() == fused_mlp.mlp3_buffers(L1, L2, Bp, "cpu")["xring"].numel()
    assert torch.equal(R.xring_dense(ring, Bp), x)
    assert float(ring.view(2, 49, Bp, 16)[1, 5, 3, 2]) == float(x[1, 3, 5 * 16 + 2])
    d = {k: torch.randn(Bp, n, generator=g).to(torch.bfloat16).double()
         for k, n in (("h1", L1), ("h2", L2), ("dh2", L2), ("dz", 16), ("dh1", L1))}
    act, dh1t = R.act_pack(d, L1, L2)
    bufs = fused_mlp.mlp3_buffers(L1, L2, Bp, "cpu")
    assert act.numel() == bufs["act"].numel() and dh1t.numel() == bufs["dh1t"].numel()
    back = R.act_dense(act, dh1t, L1, L2, Bp)
    assert all(torch.equal(back[k], d[k]) for k in d)
    assert float(act.view(-1, Bp)[R.act_rows(L1, L2)["DZT"] + 2, 7]) == float(d["dz"][7, 2])


def test_test_mlp3_keeps_the_same_h1pre_map():
    import test_mlp3 as T

    slot = torch.randint(-2 ** 25, 2 ** 25, (32 * 64,), dtype=torch.int32)
    assert torch.equal(T._h1pre_dense(slot, 64), R.h1pre_dense(slot, 64, 32).double() / R.FIX)
