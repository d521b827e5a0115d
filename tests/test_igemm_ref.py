"""CPU checks of the contraction test helpers (tests/igemm_ref.py): the float64 reference against torch's own fp32 operators, the
buffer helpers, and the statement that the cases of tests/test_gpu_igemm_ops.py can tell a right kernel from a wrong one -- on
the very inputs the GPU cases use, each targeted mistake moves the result further than FAR x the loosest gate a case is held
to (bf16x3, 2e-4), while the fp32 torch restatement of the same case stays within a quarter of the tightest (2e-5), so no gate
needs widening for the tanh / erf cases."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import igemm_ref as R

LOOSEST = max(R.GATE.values())
TIGHTEST = min(R.GATE.values())
FAR = 10.0


def _nchw(buf, B, H, W, ld, C):
    return R.rows_of(buf, B * H * W, ld, C).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def _rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


@pytest.mark.parametrize("spec", [
    dict(k=3, Cout=24, bias=True),
    dict(k=1, Cout=24, bias=True, act=3),
    dict(k=3, Cout=24, C2=8, ld1_pad=4, a_leaky=0.2, act=1),
    dict(k=3, Cout=24, up=1, bias=True, act=4),
])
def test_reference_against_torch_fp32(spec):
    """conv2d / interpolate / leaky_relu / gelu / tanh of torch in fp32 on the concatenated NCHW tensor."""
    B, H, W, C1 = 2, 5, 6, 16
    c = R.Case(B=B, H=H, W=W, C1=C1, seed=3, **spec)
    x = _nchw(c.x1, B, H, W, c.ld1, C1)
    if c.C2:
        x = torch.cat([x, _nchw(c.x2, B, H, W, c.ld2, c.C2)], dim=1)
    if spec.get("up"):
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if spec.get("a_leaky"):
        x = F.leaky_relu(x, spec["a_leaky"])
    y = F.conv2d(x, c.w, c.bias, padding=spec["k"] // 2)
    act = spec.get("act", 0)
    y = {0: lambda t: t, 1: torch.tanh, 3: F.gelu, 4: lambda t: F.leaky_relu(t, R.SLOPE)}[act](y)
    got, _ = c.reference("f32")
    assert got.dtype == torch.float64 and R.rel_max(got, _rows(y).double()) < 2e-6


def test_reference_geometry_stride_dilation_one_sided_padding():
    """stride 2 with zeros on the right / bottom only (the VAE's downsample), dilation with "same" padding, and pad_h apart
    from pad_w (a 1-D kernel over the width)."""
    B, H, W, C, N = 2, 6, 8, 8, 12
    x = torch.randn(B, H, W, C, generator=R.gen(1))
    xn = x.permute(0, 3, 1, 2)
    w = torch.randn(N, C, 3, 3, generator=R.gen(2))
    none = torch.zeros(0)
    got, _ = R.igemm_ref(x, C, C, None, 0, 0, B, H, W, 3, 4, w, None, none, N, stride=2, pad_w=0, pad_h=0)
    assert R.rel_max(got, _rows(F.conv2d(F.pad(xn, (0, 1, 0, 1)), w, stride=2)).double()) < 2e-6
    got, _ = R.igemm_ref(x, C, C, None, 0, 0, B, H, W, H, W, w, None, none, N, pad_w=2, dil=2)
    assert R.rel_max(got, _rows(F.conv2d(xn, w, padding=2, dilation=2)).double()) < 2e-6
    w1 = torch.randn(N, C, 1, 5, generator=R.gen(3))
    got, _ = R.igemm_ref(x, C, C, None, 0, 0, B, H, W, H, W, w1, None, none, N, pad_w=2)
    assert R.rel_max(got, _rows(F.conv2d(xn, w1, padding=(0, 2))).double()) < 2e-6


def test_reference_epilogue_order_and_geglu():
    """((alpha acc + bias + rowadd + res) -> act) * out_scale + c, c2 = leaky of that; GEGLU = value * gelu(gate) with the value in
    the first half of the weight's rows -- spelled out with torch's fp32 operators."""
    c = R.Case(B=3, H=2, W=3, C1=16, Cout=32, k=1, seed=4, c2=True, **dict(R.ALL_TERMS, act=3))
    a = R.rows_of(c.x1, c.M, c.ld1, 16)
    ra = R.rows_of(c.rowadd, 3, c.ld_rowadd, 32).repeat_interleave(6, dim=0)
    v = F.linear(a, c.w[:, :, 0, 0]) * 0.5 + c.bias + ra + R.rows_of(c.res, c.M, c.ldr, 32)
    v = F.gelu(v) * (1.0 / 3.0) + c.prior
    got, got2 = c.reference("f32")
    assert R.rel_max(got, v.double()) < 2e-6 and R.rel_max(got2, F.leaky_relu(v, R.SLOPE).double()) < 2e-6
    g = R.Case(B=1, H=1, W=7, C1=32, Cout=128, geglu=True, seed=5, alpha=0.5)
    val, gate = (F.linear(R.rows_of(g.x1, 7, 32, 32), g.w) * 0.5 + g.bias).chunk(2, dim=-1)
    assert g.N == 64 and R.rel_max(g.reference("f32")[0], (val * F.gelu(gate)).double()) < 2e-6


def test_plain_bf16_rounds_the_operands_after_the_activation():
    c = R.Case(B=1, H=1, W=9, C1=32, Cout=32, a_leaky=0.3, seed=6)
    a = F.leaky_relu(R.rows_of(c.x1, 9, 32, 32), 0.3).to(torch.bfloat16).double()
    ref = a @ c.w[:, :, 0, 0].to(torch.bfloat16).double().t()
    assert R.rel_max(c.reference("bf16")[0], ref) < 1e-12
    assert R.rel_max(c.reference("bf16")[0], c.reference("f32")[0]) > 1e-4      # ... and that is a different problem


def test_buffers():
    """Inputs: the large finite fill everywhere outside the rows' columns.  Outputs: one bit pattern; outside_untouched sees a
    single changed float in the pitch padding, in the spare rows and in front of the base, and none inside the result."""
    x = torch.randn(5, 6, generator=R.gen(7))
    buf = R.padded_in(x, 8, lead=1)
    assert buf.numel() == 41 and torch.equal(R.rows_of(buf[1:], 5, 8, 6), x)
    assert float(buf[0]) == R.FILL_IN and bool((R.rows_of(buf[7:], 4, 8, 2) == R.FILL_IN).all()) and bool(torch.isfinite(buf).all())
    prior = torch.randn(5, 6, generator=R.gen(8))
    out = R.out_buffer(5, 6, 8, lead=1, prior=prior)
    assert out.numel() == 1 + (5 + R.SPARE_ROWS) * 8 and torch.equal(R.rows_of(out[1:], 5, 8, 6), prior)
    assert R.outside_untouched(out, 5, 6, 8, lead=1)
    R.rows_of(out[1:], 5, 8, 6).fill_(1.0)
    assert R.outside_untouched(out, 5, 6, 8, lead=1)
    for at in (0, 1 + 6, 1 + 4 * 8 + 7, 1 + 5 * 8, out.numel() - 1):
        bad = out.clone()
        bad[at] = 0.0
        assert not R.outside_untouched(bad, 5, 6, 8, lead=1), at
    x = torch.randn(4, 64, generator=R.gen(9))
    assert R.rel_max(R.split32_decode(R.split32_encode(x, 72), 4, 64), x.double()) < 2.0 ** -15


# ------------------------------------------------------------------------------------------------ the GPU cases can tell
def _moved(c, mistake, second=False):
    i = 1 if second else 0
    return min(R.rel_max(c.reference(p, mistake)[i], c.reference(p)[i]) for p in R.GATE)


def test_term_cases_show_each_mistake():
    """Group (a).  out_scale in front of the activation is a mistake only where the activation is not positively homogeneous:
    relu and leaky-relu commute with a positive scale, so for them the two orders are the same function."""
    seen = set()
    for name, c in R.term_cases():
        if name.startswith("rowadd") or name.startswith("all_act"):
            for m in ("rowadd_next_sample", "rowadd_pitch_n"):
                assert _moved(c, m) > FAR * LOOSEST, (name, m)
                seen.add(m)
        if name.startswith("all_act") and c.kw["act"] != 0:
            assert _moved(c, "act_before_res") > FAR * LOOSEST, name
            seen.add("act_before_res")
            if c.kw["act"] in (1, 3):
                assert _moved(c, "scale_before_act") > FAR * LOOSEST, name
                seen.add("scale_before_act")
            else:
                assert _moved(c, "scale_before_act") < 1e-12, name
    assert seen == {"rowadd_next_sample", "rowadd_pitch_n", "act_before_res", "scale_before_act"}


def test_the_fp32_restatement_is_well_inside_the_gates():
    """Every group (a) case in fp32 torch against the float64 reference: at most a quarter of the tightest gate, tanh and erf
    included (measured: 1.5e-6 at the worst case), so max(gate, 4 x this) is the gate itself."""
    worst = 0.0
    for name, c in R.term_cases():
        worst = max(worst, R.rel_max(c.reference("f32", dtype=torch.float32)[0].double(), c.reference("f32")[0]))
    print("fp32 restatement, worst rel-max over group (a): %.3e" % worst)
    assert 4 * worst <= TIGHTEST


def test_second_output_cases_show_a_pre_activation_source():
    for B, H, W in R.IMAGES:
        for k in R.KERNELS:
            c = R.case(B=B, H=H, W=W, C1=R.CIN, Cout=96, k=k, seed=13, **R.SPLIT_OUTS["c2_leaky"])
            assert _moved(c, "c2_pre_act", second=True) > FAR * LOOSEST


def test_geglu_cases_show_exchanged_halves():
    for M in R.GEGLU_M:
        for packed in R.GEGLU_PACKED:
            for K in R.GEGLU_K:
                c = R.case(B=1, H=1, W=M, C1=K, Cout=packed, geglu=True, seed=14)
                assert _moved(c, "geglu_halves") > FAR * LOOSEST


def test_two_source_cases_show_swapped_sources():
    """Random weights and the one-hot probes: with the sources exchanged every plane of the probe is another channel's."""
    for C1, C2 in R.TWO_SOURCES + R.TWO_SOURCES_UNALIGNED:
        for k in R.KERNELS:
            B, H, W = R.IMAGES[0]
            c = R.case(B=B, H=H, W=W, C1=C1, C2=C2, ld1_pad=R.LD1_PAD, Cout=96, k=k, seed=15)
            assert _moved(c, "sources_swapped") > FAR * LOOSEST
            for tap in range(k * k):
                p = R.Case(B=B, H=H, W=W, C1=C1, C2=C2, ld1_pad=R.LD1_PAD, Cout=C1 + C2, k=k, seed=15,
                           weight=R.one_hot_weight(C1 + C2, k, tap))
                ref = p.reference("f32")[0]
                wrong = p.reference("f32", "sources_swapped")[0]
                assert float((ref - wrong).abs().max()) > 0.5
                # the probe copies: plane n is channel n of the concatenation, shifted by the tap, exactly
                x = torch.cat([R.rows_of(p.x1, p.M, p.ld1, C1), R.rows_of(p.x2, p.M, p.ld2, C2)], 1).reshape(B, H, W, -1)
                dy, dx = tap // k - k // 2, tap % k - k // 2
                shifted = F.pad(x.permute(0, 3, 1, 2), (k, k, k, k))[:, :, k + dy:k + dy + H, k + dx:k + dx + W]
                assert torch.equal(ref, _rows(shifted).double())
