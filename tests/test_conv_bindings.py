"""Refusals of the convolution bindings (csrc/bindings.cpp): a bad operand is an exception
raised before any launch, whichever binding it is handed to.

Every case starts from a binding's smallest valid argument list and breaks one thing: a
bf16 operand on the CPU, in fp32, as a non-contiguous view, as a view that starts one
element (2 bytes) into its storage, with one row too few, or (two GPUs) on the other
device; the BatchNorm statistics as [4, C + 1] or [C, 4]; the ``num_batches_tracked``
counter empty.  No case launches a kernel: the valid lists themselves are only checked
against the bindings' host-side predicates.
"""
import pytest
import torch

gpu = pytest.mark.gpu


def _ops():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _bf16(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device="cuda:0")


def _ss(c):
    return torch.zeros(4, c, dtype=torch.float32, device="cuda:0")


def _nbt():
    return torch.zeros((), dtype=torch.int64, device="cuda:0")


C3 = (1, 4, 4, 16, 64)                             # 3x3: N, H, W, Cin, Cout
WG = (1, 4, 4, 64, 4, 4, 64, 3, 3, 1, 1, 1, 1)     # wgrad: 3x3 / stride 1 / pad 1 over 64 -> 64 channels
M1, K1, N1 = 128, 32, 64                           # 1x1: x [M, K], w [N, K]

# binding -> (operands by name, in call order; call(module, operands); the operands whose size the
#             others fix; (statistics operand, its C); the counter operand)
BINDINGS = {
    "conv_wgrad": (lambda: {"dy": _bf16(1, 4, 4, 64), "x": _bf16(1, 4, 4, 64), "pre_ss": _ss(64)},
                   lambda m, o: m.conv_wgrad(o["dy"], o["x"], *WG, 0, 0, o["pre_ss"]),
                   ("dy", "x"), ("pre_ss", 64), None),
    "conv3x3": (lambda: {"x": _bf16(1, 4, 4, 16), "w": _bf16(64, 3, 3, 16)},
                lambda m, o: m.conv3x3(o["x"], o["w"], *C3),
                ("x", "w"), None, None),
    "conv3x3_stats": (lambda: {"x": _bf16(1, 4, 4, 16), "w": _bf16(64, 3, 3, 16), "pre_ss": _ss(16), "nbt_inc": _nbt()},
                      lambda m, o: m.conv3x3_stats(o["x"], o["w"], *C3, o["pre_ss"], o["nbt_inc"]),
                      ("x", "w"), ("pre_ss", 16), "nbt_inc"),
    "conv3x3_dgrad_bn": (lambda: {"dy": _bf16(1, 4, 4, 16), "w": _bf16(16, 3, 3, 64), "xb": _bf16(1, 4, 4, 64),
                                  "ss": _ss(64)},
                         lambda m, o: m.conv3x3_dgrad_bn(o["dy"], o["w"], *C3, o["xb"], o["ss"]),
                         ("dy", "w", "xb"), ("ss", 64), None),
    "conv3x3s2": (lambda: {"x": _bf16(1, 4, 4, 16), "w": _bf16(64, 3, 3, 16)},
                  lambda m, o: m.conv3x3s2(o["x"], o["w"], *C3),
                  ("x", "w"), None, None),
    "conv3x3s2_stats": (lambda: {"x": _bf16(1, 4, 4, 16), "w": _bf16(64, 3, 3, 16)},
                        lambda m, o: m.conv3x3s2_stats(o["x"], o["w"], *C3),
                        ("x", "w"), None, None),
    # the stem kernels take N, H, W from x: one row less of x is another valid input
    "stem_fwd": (lambda: {"x": _bf16(1, 8, 8, 3), "w": _bf16(64, 7, 7, 3)},
                 lambda m, o: m.stem_fwd(o["x"], o["w"], True),
                 ("w",), None, None),
    "stem_wgrad": (lambda: {"x": _bf16(1, 8, 8, 3), "dy": _bf16(1, 4, 4, 64)},
                   lambda m, o: m.stem_wgrad(o["x"], o["dy"]),
                   ("dy",), None, None),
    # M is x's row count: one row less of x is another valid input; of w, N = 63
    "conv1x1_stats": (lambda: {"x": _bf16(M1, K1), "w": _bf16(N1, K1), "pre_ss": _ss(K1), "nbt_inc": _nbt()},
                      lambda m, o: m.conv1x1_stats(o["x"], o["w"], o["pre_ss"], o["nbt_inc"]),
                      ("w",), ("pre_ss", K1), "nbt_inc"),
    "conv1x1_bn_bwd": (lambda: {"dy1": _bf16(M1, K1), "wt": _bf16(N1, K1), "dy2": _bf16(M1, N1), "yb": _bf16(M1, N1),
                                "xb": _bf16(M1, N1)},
                       lambda m, o: m.conv1x1_bn_bwd(o["dy1"], o["wt"], o["dy2"], o["yb"], o["xb"]),
                       ("dy1", "wt", "dy2", "yb", "xb"), None, None),
    # the pool takes every size from x
    "maxpool_fwd": (lambda: {"x": _bf16(1, 8, 8, 64), "bn_ss": _ss(64), "nbt_inc": _nbt()},
                    lambda m, o: m.maxpool_fwd(o["x"], 3, 2, 1, o["bn_ss"], o["nbt_inc"]),
                    (), ("bn_ss", 64), "nbt_inc"),
}


def _break(t, how):
    if how == "cpu":
        return t.cpu()
    if how == "fp32":
        return t.float()
    if how == "noncontiguous":  # same shape and element count, every other element of a wider buffer
        wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
        v = wide[..., ::2]
        assert v.shape == t.shape and not v.is_contiguous() and v.data_ptr() % 16 == 0
        return v
    if how == "offset":  # contiguous, the right size, 2 bytes off every wider alignment
        v = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 4 == 2
        return v
    if how == "numel":
        return t[:-1].contiguous() if t.size(0) > 1 else t[:, :-1].contiguous()
    if how == "other_device":
        return t.to("cuda:1")
    raise AssertionError(how)


# the bf16 operands of each binding, the first one first (the device every other is compared with)
_OPERANDS = {
    "conv_wgrad": ("dy", "x"), "conv3x3": ("x", "w"), "conv3x3_stats": ("x", "w"),
    "conv3x3_dgrad_bn": ("dy", "w", "xb"), "conv3x3s2": ("x", "w"), "conv3x3s2_stats": ("x", "w"),
    "stem_fwd": ("x", "w"), "stem_wgrad": ("x", "dy"), "conv1x1_stats": ("x", "w"),
    "conv1x1_bn_bwd": ("dy1", "wt", "dy2", "yb", "xb"), "maxpool_fwd": ("x",),
}


def _cases():
    out = []
    for name, (_, _, sized, ss, nbt) in BINDINGS.items():
        ops = _OPERANDS[name]
        for op in ops:
            for how in ("cpu", "fp32", "noncontiguous", "offset"):
                out.append((name, op, how))
            if op in sized:
                out.append((name, op, "numel"))
            if op != ops[0]:
                out.append((name, op, "other_device"))
        if ss is not None:
            out += [(name, ss[0], "ss_c_plus_1"), (name, ss[0], "ss_transposed"), (name, ss[0], "other_device")]
        if nbt is not None:
            out.append((name, nbt, "nbt_empty"))
    return out


@gpu
def test_base_argument_lists_are_valid():
    """The lists the refusal cases start from are ones the bindings take (host-side
    predicates and plan queries only): a case's exception is its one broken operand's."""
    m = _ops()
    assert m.conv3x3_supported(*C3) and m.conv3x3s2_supported(*C3) and m.conv3x3_dgrad_bn_ok(*C3)
    assert m.conv3x3_plan(*C3, False, True, True)  # pre_ss on the statistics forward
    assert m.stem_supported(1, 8, 8) and m.stem_grid(1, 8, 8) >= 1
    assert m.conv1x1_stats_ok(M1, K1, N1) and m.conv1x1_pre_ok(M1, K1, N1) and m.conv1x1_bn_bwd_ok(M1, K1, N1)
    assert len(m.conv_wgrad_plan(*WG, 0, 0)) == 5
    assert set(_OPERANDS) == set(BINDINGS)


@gpu
@pytest.mark.parametrize("name,operand,how", _cases(), ids=lambda v: str(v))
def test_bad_operand_is_refused_before_any_launch(name, operand, how):
    make, call, _, ss, _ = BINDINGS[name]
    if how == "other_device" and torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    m = _ops()
    ops = make()
    if how == "ss_c_plus_1":
        ops[operand] = _ss(ss[1] + 1)
    elif how == "ss_transposed":
        ops[operand] = torch.zeros(ss[1], 4, dtype=torch.float32, device="cuda:0")
    elif how == "nbt_empty":
        ops[operand] = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    else:
        ops[operand] = _break(ops[operand], how)
    with pytest.raises(RuntimeError):
        call(m, ops)
