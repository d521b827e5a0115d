"""CPU checks of the normalisation tests' yardsticks (tests/norm_ref.py): the float64 references against torch's own
group_norm / layer_norm in float64, the layout plan against the table of shapes, and the input condition -- on every input the
GPU tests use, torch's fp32 group_norm / layer_norm on the CPU stays within HALF of the tolerance of the float64 reference under
the metric the GPU test applies (whole tensor, and the elements that were not planted relative to their own maximum), so a
correct fp32 kernel has room and a miss on the GPU is the kernel's."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R


def _cl(x):
    """channels-last [B, HW, C] -> torch's [B, C, HW]"""
    return x.permute(0, 2, 1).contiguous()


def _torch_gn(x, gamma, beta, eps, silu, dtype):
    y = F.group_norm(_cl(x).to(dtype), R.GROUPS, gamma.to(dtype), beta.to(dtype), eps)
    return (F.silu(y) if silu else y).permute(0, 2, 1)


def test_groupnorm_ref_matches_torch_float64():
    for C1, C2, HW in ((64, 32, 77), (12, 20, 5), (320, 640, 50)):
        x = R.gn_input(2, C1 + C2, HW)
        ga, be = R.gn_params(C1 + C2)
        for eps, silu in R.GN_VARIANTS:
            ref = R.groupnorm_ref(R.split_sources(x, C1), R.GROUPS, ga, be, eps, silu)
            assert R.rel_max(ref, _torch_gn(x, ga, be, eps, silu, torch.float64)) < 1e-13


def test_layernorm_ref_matches_torch_float64():
    for rows, C in ((9, 768), (1, 4)):
        for kind in R.LN_KINDS:
            x, _ = R.ln_input(rows, C, kind)
            ga, be = R.ln_params(C)
            for eps in R.LN_EPS:
                t = F.layer_norm(x.double(), (C,), ga.double(), be.double(), eps)
                assert R.rel_max(R.layernorm_ref(x, ga, be, eps), t) < 1e-12


def test_shapes_reach_the_kernels_they_are_listed_for():
    for (C, HW), plan in R.GN_SHAPES.items():
        assert R.fused_plan(C, HW) == plan, (C, HW, R.fused_plan(C, HW))
    assert {p[1] for p in R.GN_SHAPES.values() if p} == {1, 2, 4, 8, 12, 16}
    assert R.fused_plan(1920, 195) == (2, 8, 1020)         # the model's (1280 | 640) decoder ResBlock
    for C1, C2, HW in R.GN_SPLITS:
        assert (C1 + C2, HW) in R.GN_SHAPES or (C1, C2, HW) == (1280, 640, 195)
        assert C1 % 4 == 0 and C2 % 4 == 0
    assert any(C1 % ((C1 + C2) // R.GROUPS) for C1, C2, _ in R.GN_SPLITS)
    # both kernels among the hard shapes, and a straddling group in at least one of them
    assert any(R.fused_plan(a + b, hw) is None for a, b, hw in R.HARD_SHAPES)
    assert any(a % ((a + b) // R.GROUPS) for a, b, hw in R.HARD_SHAPES)


@pytest.mark.parametrize("C,HW", sorted(R.GN_SHAPES) + [(1920, 195)])
def test_groupnorm_inputs_leave_half_the_tolerance(C, HW):
    x = R.gn_input(R.gn_batch(C, HW), C, HW)
    ga, be = R.gn_params(C)
    for eps, silu in R.GN_VARIANTS:
        ref = R.groupnorm_ref([x], R.GROUPS, ga, be, eps, silu)
        assert R.rel_max(_torch_gn(x, ga, be, eps, silu, torch.float32), ref) <= R.GN_TOL / 2


@pytest.mark.parametrize("case", R.HARD_CASES)
@pytest.mark.parametrize("C1,C2,HW", R.HARD_SHAPES)
def test_hard_groupnorm_inputs_leave_half_the_tolerance(C1, C2, HW, case):
    x, keep = R.hard_input(C1, C2, HW, case)
    ga, be = R.gn_params(C1 + C2)
    ref = R.groupnorm_ref([x], R.GROUPS, ga, be, 1e-5, True)
    got = _torch_gn(x, ga, be, 1e-5, True, torch.float32)
    assert torch.isfinite(got).all()
    assert R.rel_max(got, ref) <= R.GN_TOL / 2
    assert R.rel_max(got, ref, keep) <= R.GN_TOL / 2
    if case == "constant":
        c = R.constant_group_slice(C1, C2)
        assert R.rel_max(ref[..., c], F.silu(be.double())[c].expand_as(ref[..., c])) < 1e-12


@pytest.mark.parametrize("rows,C", R.LN_SHAPES)
def test_layernorm_inputs_leave_half_the_tolerance(rows, C):
    ga, be = R.ln_params(C)
    for kind in R.LN_KINDS:
        x, keep = R.ln_input(rows, C, kind)
        for eps in R.LN_EPS:
            ref = R.layernorm_ref(x, ga, be, eps)
            got = F.layer_norm(x, (C,), ga, be, eps)
            assert R.rel_max(got, ref) <= R.LN_TOL / 2, (kind, eps)
            assert R.rel_max(got, ref, keep) <= R.LN_TOL / 2, (kind, eps)


def test_pack_input_holds_the_edge_values():
    x = R.pack_input(3, 32)
    assert torch.isfinite(x).all()
    bits = x.view(torch.int32)
    assert int(bits[0, 0]) == 0 and int(bits[0, 1]) == -(1 << 31)            # +0, -0
    assert 0 < abs(float(x[0, 2])) < 1.2e-38                                   # a denormal
    tie = x[0, 7]                                                              # 0x3f808000: half way between two bf16
    assert float(tie.to(torch.bfloat16)) != float(tie) and int(bits[0, 7]) & 0xffff == 0x8000
    enc = R.split32_encode(x)
    assert torch.equal(R.split32_decode(enc, 3, 32), (x.to(torch.bfloat16).double() + (x - x.to(torch.bfloat16).float()).to(torch.bfloat16).double()))
