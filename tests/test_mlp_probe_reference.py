"""The gate-and-probe method of tests/mlp_reference.py checked on the CPU, before
tests/test_mlp_step_1wg_fp64.py runs it on csrc/mlp_kernels.hip: an fp32 / bf16 emulation of the
kernel's arithmetic (``emulate_step_1wg``) passes every check of every family, each of its wrong
variants a to g fails a named check, and every committed case meets the preconditions the method
rests on -- the logit gap of the gate, the certificates of the dyadic family, no ambiguous row,
and a nonzero dZ, dH2 and dH1 factor in every probe row (nothing is skipped: the allowed share of
rows without a factor is zero)."""
import pytest
import torch

import mlp_reference as R
import test_mlp_step_1wg_fp64 as G

# small enough to sweep row by row on the CPU: both chunk sizes, the three split counts, ragged
# last chunks of one row, L2 < L1
EMU_CASES = [(32, 64, 33, "f32"), (32, 32, 65, "norm"), (64, 128, 33, "u8"), (128, 256, 33, "norm"),
             (128, 64, 33, "f32"), (32, 64, 65, "u8"), (64, 128, 40, "norm"), (32, 64, 1, "f32")]


def _emu(c, wrong=None, params=None):
    def step(order, t=1, **kw):
        out = R.emulate_step_1wg(c.params if params is None else params, c.X2[order], c.y2[order], c.B, c.BC,
                                 c.L1, c.L2, step=t, wrong=wrong, **kw)
        return out["grads"], out["stats"]
    return step


def _probe(c, wrong=None):
    """Names of the failed checks of a probe sweep + superposition of the emulation."""
    rows, stats, gsum, gabs, bad = R.probe_sweep(_emu(c, wrong), c.B, c.L1, c.L2)
    failed = [s for _, s, _ in bad]
    if rows is None:
        return failed, None
    res = R.probe_checks(rows, c.wt, c.X2[:c.B], c.y2[:c.B], c.B, exact=c.exact, stats=stats,
                         steps=torch.arange(1, c.B + 1))
    g, st = _emu(c, wrong)(torch.arange(c.B))
    res += [("super_" + s, r) for s, r in R.superposition_checks(g, gsum, gabs, c.Bp, c.L1, c.L2)]
    Z, ez = R.ref_logits(rows["h2"], c.wt.W3, c.wt.b3)
    ref = R.ref_stats(Z, ez, c.y2[:c.B])
    res.append(("super_loss", R.cmp_bound(st[:1], torch.tensor([ref.loss], dtype=torch.float64),
                                          ref.loss_bound + (c.Bp + 2) * R.U24 * ref.loss)))
    R.report(f"emulation {c.L1}/{c.L2} B={c.B} {c.family} wrong={wrong}", res)
    return failed + [s for s, r in res if not r.ok], res


def _exact(c, wrong=None):
    y = c.y2[:c.B]
    obs, cert = R.exact_batch(c.X2[c.B:], y, c.wt, c.B, c.c0)
    out = R.emulate_step_1wg(c.params, c.X2[c.B:], y, c.B, c.BC, c.L1, c.L2, wrong=wrong)
    return obs, cert, out, R.exact_batch_checks(out["grads"], obs, cert, c.L1, c.L2, c.Bp)


def test_the_case_lists_reach_every_path():
    """By the Python mirror of ``Cfg::total`` / ``fits<64>()`` / ``NSPLIT`` (which nothing the
    kernel exports can confirm): both chunk sizes, the three split counts, a last chunk of one row,
    4 and 8 chunks, the three staging instances, Adam over several chunks."""
    assert [R.chunk_rows_1wg(L1, L2, 64) for L1, L2 in G.WIDTHS] == [64, 64, 32, 32, 32]
    assert [R.chunk_rows_1wg(*s) for s in ((32, 64, 32), (32, 128, 64), (64, 64, 64))] == [32, 32, 32]
    assert R.lds_total_1wg(64, 32, 64) == 153152
    for cases in (G.PROBE_CASES, [c + ("norm",) for c in G.EXACT_CASES], G.SUPER_CASES):
        seen = {(R.chunk_rows_1wg(L1, L2, B), R.nsplit_1wg(L1)) for L1, L2, B, _ in cases if B > 32}
        assert seen == {(64, 4), (32, 2), (32, 1)}, seen
        shape = {(B % R.chunk_rows_1wg(L1, L2, B), -(-B // R.chunk_rows_1wg(L1, L2, B))) for L1, L2, B, _ in cases}
        assert {1, 4, 8} <= {n for _, n in shape} and any(last == 1 and n > 1 for last, n in shape), shape
    assert {f for *_, f in G.PROBE_CASES} == {"f32", "norm", "u8"}
    assert all(-(-B // R.chunk_rows_1wg(L1, L2, B)) >= 2 for L1, L2, B, _ in G.ADAM_CASES)
    assert {R.chunk_rows_1wg(L1, L2, B) for L1, L2, B, _ in G.ADAM_CASES} == {32, 64}
    assert any(B % R.chunk_rows_1wg(L1, L2, B) for L1, L2, B, _ in G.ADAM_CASES)


@pytest.mark.parametrize("L1,L2,B,family", G.committed_cases())
def test_committed_cases_meet_the_preconditions(L1, L2, B, family):
    """Rows are independent, so one emulated step over the gate-off batch shows every probe row's
    factors; the sweep itself is emulated for the small cases below."""
    c = G.make_case(L1, L2, B, family)
    assert R.gate_gap(c.X2[B:], c.wt, c.c0) >= R.GAP_MIN          # derived: expf underflows below about -104
    out = R.emulate_step_1wg(c.params, c.X2[:B], c.y2[:B], B, c.BC, L1, L2)
    rows = {k: v[:B] for k, v in out["rows"].items()}
    for k in ("dz", "dh2", "dh1"):
        assert bool((rows[k] != 0).any(1).all()), f"a probe row without a {k} factor"
    assert float(rows["dz"][B:].abs().sum() if B < c.Bp else 0.0) == 0.0
    silent = R.emulate_step_1wg(c.params, c.X2[B:], c.y2[B:], B, c.BC, L1, L2)
    assert float(silent["grads"].abs().sum()) == 0.0 and silent["stats"].tolist() == [0.0, B, B, 1.0]
    Z, ez = R.ref_logits(rows["h2"], c.wt.W3, c.wt.b3)
    if c.exact:
        assert R.exact_certificate(c.X2, c.wt.W1, c.wt.b1).ok and R.exact_certificate(rows["h1"], c.wt.W2, c.wt.b2).ok
        if R.exact_certificate(rows["h2"], c.wt.W3, c.wt.b3).ok:
            ez = torch.zeros_like(ez)
    assert R.ref_stats(Z, ez, c.y2[:B]).ambiguous == 0
    assert int(R.row_nll(Z, ez, c.y2[:B])[3].sum()) == 0


@pytest.mark.parametrize("L1,L2,B", G.EXACT_CASES)
def test_exact_batch_is_certified_and_the_emulation_reproduces_it(L1, L2, B):
    c = G.make_case(L1, L2, B, "norm")
    obs, cert, out, res = _exact(c)
    assert all(cert[k] for k in ("H1", "H2", "dH2", "dH1")), cert
    assert {"d" + k for k in R.NAMES if cert["d" + k]} == G.exact_grads(B), cert
    print(f"[certificate] exact {L1}/{L2} B={B}: " + " ".join(k for k, v in cert.items() if v))
    for k in ("h1", "h2", "dz", "dh2", "dh1"):
        assert torch.equal(out["rows"][k][:B], obs[k]), k
    assert not R.report(f"exact {L1}/{L2} B={B}", res), res
    assert out["stats"][1:].tolist() == [float((c.y2[:B] == c.c0).sum()), B, 1.0]


@pytest.mark.parametrize("L1,L2,B,family", EMU_CASES)
def test_emulation_passes_every_check(L1, L2, B, family):
    failed, res = _probe(G.make_case(L1, L2, B, family))
    assert failed == [] and res is not None, failed


def test_a_loud_gate_on_row_is_recovered_exactly():
    """Gate on with a label other than c0: dZ is exactly bf16(+-1 / B) at c0 and at the label."""
    c = G.make_case(64, 128, 40, "norm")
    y2 = c.y2.clone()
    y2[c.B + 5] = (c.c0 + 1) % 10
    out = R.emulate_step_1wg(c.params, c.X2[c.B:], y2[c.B:], c.B, c.BC, c.L1, c.L2)
    row, res = R.recover_row(out["grads"], c.L1, c.L2)
    assert all(r.ok for _, r in res), res
    inv = float((torch.tensor(1.0) / torch.tensor(40.0)).to(torch.bfloat16))
    want = torch.zeros(16, dtype=torch.float64)
    want[c.c0], want[c.c0 + 1] = inv, -inv
    assert torch.equal(row["dz"], want) and torch.equal(row["x"], c.X2[c.B + 5])


def test_row_nll_is_ref_stats_row_by_row():
    c = G.make_case(32, 64, 33, "f32")
    Z, ez = R.ref_logits(R.forward_fp64(c.X2[:33], c.wt)[1], c.wt.W3, c.wt.b3)
    nll, bound, sure, amb = R.row_nll(Z, ez, c.y2[:33])
    st = R.ref_stats(Z, ez, c.y2[:33])
    assert abs(float(nll.mean()) - st.loss) < 1e-12 and abs(float(bound.mean()) - st.loss_bound) < 1e-15
    assert int(sure.sum()) == st.certain and int(amb.sum()) == st.ambiguous


# ------------------------------------------------------------------ mutants
def _adam_failed(c, wrong=None, cfg=G.ADAM_CFGS[1], t=2):
    n = c.params.numel()
    v0 = torch.rand(n, generator=torch.Generator().manual_seed(3)) * 1e-4
    adam = dict(m=torch.zeros(n), v=v0, lr=cfg.lr, betas=cfg.betas, eps=cfg.eps, wd=cfg.wd, adamw=cfg.adamw)
    order = torch.arange(c.B)
    plain = R.emulate_step_1wg(c.params, c.X2[order], c.y2[order], c.B, c.BC, c.L1, c.L2, step=t)
    out = R.emulate_step_1wg(c.params, c.X2[order], c.y2[order], c.B, c.BC, c.L1, c.L2, adam=adam, step=t, wrong=wrong)
    res = R.adam_checks({"p": c.params, "v": v0}, out, plain["grads"], cfg, t)
    R.report(f"adam emulation wrong={wrong}", res)
    return [s for s, r in res if not r.ok]


@pytest.mark.parametrize("cfg", G.ADAM_CFGS, ids=lambda c: c.name)
def test_emulated_adam_on_the_last_chunk_passes(cfg):
    for shape in ((32, 64, 100, "f32"), (64, 128, 40, "norm")):
        assert _adam_failed(G.make_case(*shape), cfg=cfg) == []


@pytest.mark.parametrize("wrong,case,named", [
    ("a", (64, 128, 40, "f32"), {"speaks", "super_dW1"}),    # a first-chunk row's gradient is wiped
    ("b", (32, 64, 65, "u8"), {"dZ"}),
    ("c", (64, 128, 33, "norm"), {"dH1"}),
    ("d", (32, 64, 33, "f32"), {"rank1_W3"}),                # 31 padded rows leak
    ("e", (128, 64, 33, "f32"), {"rank1_W1"}),
    ("g", (64, 128, 40, "norm"), {"speaks", "super_db1"}),   # a second-chunk row has no db
], ids=lambda v: v if isinstance(v, str) else None)
def test_wrong_variants_fail_a_named_check(wrong, case, named):
    assert wrong in R.WRONG_1WG
    c = G.make_case(*case)
    failed, _ = _probe(c, wrong)
    print(f"[mutant {wrong}] {R.WRONG_1WG[wrong]}: {sorted(set(failed))}")
    assert named & set(failed), failed
    if c.exact:                                              # and the exact batch sees it too
        obs, cert, out, res = _exact(c, wrong)
        assert [s for s, r in res if not r.ok] or not all(torch.equal(out["rows"][k][:c.B], obs[k]) for k in obs)


def test_adam_on_every_chunk_fails_the_adam_checks():
    failed = _adam_failed(G.make_case(64, 128, 40, "f32"), wrong="f")
    assert "adam_m" in failed and "adam" in failed, failed


def test_recover_row_refuses_a_silent_batch():
    c = G.make_case(32, 64, 33, "f32")
    g, _ = _emu(c)(R.probe_order(33))
    row, res = R.recover_row(g, 32, 64)
    assert row is None and [(s, r.ok) for s, r in res] == [("speaks", False)]
