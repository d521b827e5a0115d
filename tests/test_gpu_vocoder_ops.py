"""Operator-level parity of the 1-D vocoder kernels against float64 references (tests/vocoder_ref.py), at the shapes and
edges where they can go wrong, through the dispatch the generators run:

  snake_aa_tiled_kernel<32> / <64>, snake_aa_kernel      test_snake_*
  halo_pair_bf16x3<32> / <64> (and its two-launch and implicit-GEMM fallbacks)       test_mrf_pair_*, test_halo_switching_*
  halo_conv1d_bf16x3<32> / <64> with residual, out_scale, accumulate                 test_resblock2_step_*, test_halo_switching_*
  polyphase ConvTranspose1d, U = k / s = 1, 2, 3                                     test_conv_transpose1d_*

Tolerances: snake 1e-5 rel-max; contractions 2e-5 (f32) and 2e-4 (bf16x3), the project's operator tolerances."""
import os

import pytest
import torch

from tests import vocoder_ref as R
from tests.util import check, record, rel_err

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "bf16x3")


@pytest.fixture(scope="module")
def ctxs():
    from audiogpt_amd.backend import Context
    c = {p: Context("cuda:0", precision=p) for p in PRECISIONS}
    yield c
    for v in c.values():
        v.close()


# ---------------------------------------------------------------------------------------------------------------- snake
@pytest.mark.parametrize("logscale", [True, False])
@pytest.mark.parametrize("C", R.SNAKE_TILED_C + R.SNAKE_UNTILED_C)
def test_snake_shapes_and_edges(ctxs, C, logscale):
    """Every tile count and tail (L around 64 and 128, L below the 12-tap filter), tiled and untiled; the spike input puts 50 at
    both ends and on both sides of the first tile boundary."""
    ctx = ctxs["f32"]
    for L in R.SNAKE_L:
        for kind in ("randn", "spike"):
            x, al, be, ref = R.snake_case(C, L, kind, logscale)
            check(f"vocop_snake_C{C}_L{L}_{kind}_log{int(logscale)}", ctx.op_snake_aa(x, al, be, logscale), ref, R.SNAKE_TOL)


@pytest.mark.parametrize("L", R.SNAKE_BITWISE_L)
@pytest.mark.parametrize("Ct,Cu", R.SNAKE_BITWISE)
def test_snake_tiled_is_bit_identical_to_untiled(ctxs, Ct, Cu, L):
    """misc.hip promises the tiled kernel the untiled kernel's arithmetic and summation order; channels are independent, so the
    first Cu channels of a tiled run equal an untiled run on those channels."""
    ctx = ctxs["f32"]
    for kind in ("randn", "spike"):
        x, al, be, ref = R.snake_case(Ct, L, kind, True)
        tiled = ctx.op_snake_aa(x, al, be, True).cpu()
        untiled = ctx.op_snake_aa(x[:, :Cu].contiguous(), al[:Cu], be[:Cu], True).cpu()
        check(f"vocop_snake_bitwise_C{Ct}_{Cu}_L{L}_{kind}", untiled, ref[:, :Cu], R.SNAKE_TOL)
        assert torch.equal(tiled[:, :Cu], untiled)


@pytest.mark.parametrize("C", [64, 32, 48])
def test_snake_batch_invariance(ctxs, C):
    ctx = ctxs["f32"]
    x, al, be, _ = R.snake_case(C, 129, "randn", True)
    assert torch.equal(ctx.op_snake_aa(x[1:2].contiguous(), al, be, True).cpu(), ctx.op_snake_aa(x, al, be, True).cpu()[1:2])


@pytest.mark.parametrize("C", [64, 48])
def test_snake_large_arguments(ctxs, C):
    """alpha * up up to several hundred radians (x ~ 20 randn, alpha = 10): fp32 rounding of the argument and the device's sinf
    dominate, so the bound is max(1e-5, 4 x the rel-max error of the fp32 CPU restatement against the float64 reference) -- 4 x for
    a different sinf and FMA contraction.  Measured: the fp32 CPU restatement is at 1.1e-6 (C = 64) and 1.0e-6 (C = 48), so the
    bound is 1e-5; the device is at 1.16e-6 (C = 64) and 1.03e-6 (C = 48)."""
    ctx = ctxs["f32"]
    x, al, be = R.snake_large_case(C)
    ref = R.snake_aa_ref(x, al, be, False)
    base = rel_err(R.snake_fp32_restatement(x, al, be, False), ref)[0]
    bound = max(1e-5, 4 * base)
    record(f"vocop_snake_large_C{C}_cpu_fp32_baseline", rel_max=base, bound=bound)
    check(f"vocop_snake_large_C{C}", ctx.op_snake_aa(x, al, be, False), ref, bound)


# ------------------------------------------------------------------------------------------------ MRF pair / single conv
def _run_case(ctx, C, k1, d1, k2, d2, L, kind, out_scale, acc):
    (x, w1, b1, w2, b2, prev), ref = R.mrf_case(C, k1, d1, k2, d2, L, kind, out_scale, acc)
    y = ctx.op_mrf_pair(x, w1, b1, d1, R.SLOPE, w2, b2, d2, R.SLOPE, out_scale, prev if acc else None)
    return y.cpu(), ref


def _name(precision, C, k1, d1, k2, d2, L, kind, out_scale, acc):
    return f"vocop_mrf_{precision}_C{C}_k{k1}d{d1}_k{k2}d{d2}_L{L}_{kind}_s{out_scale:.2f}_acc{int(acc)}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k1,d1,k2,d2", R.MRF_PAIRS)
@pytest.mark.parametrize("C", R.MRF_C)
def test_mrf_pair_lengths_and_epilogues(ctxs, C, k1, d1, k2, d2, precision):
    """One ResBlock1 step at one row, two rows, one row short of a tile, a tile, a tile and a one-row tail, two tiles and a
    one-row tail; three samples, so sample boundaries fall inside the persistent tile walk; every epilogue."""
    for L in R.mrf_lengths(C, k2, d2):
        for out_scale, acc in R.MRF_EPILOGUES:
            y, ref = _run_case(ctxs[precision], C, k1, d1, k2, d2, L, "randn", out_scale, acc)
            check(_name(precision, C, k1, d1, k2, d2, L, "randn", out_scale, acc), y, ref, R.TOL[precision])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k1,d1,k2,d2", R.MRF_PAIRS)
@pytest.mark.parametrize("C", R.MRF_C)
def test_mrf_pair_intermediate_is_zero_outside_the_sample(ctxs, C, k1, d1, k2, d2, precision):
    """b1 = 3: c2 must see zeros outside [0, L), not c1(0) + b1 (tests/test_vocoder_ref.py shows that this moves the first and last
    (k2 - 1) / 2 outputs of every sample by O(1)).  Then the spike input: 100 at the last position of sample 0 and the first of
    sample 1 -- nothing may cross the sample boundary inside a tile walk, and sample 2 is the answer for an all-zero sample."""
    ctx, L = ctxs[precision], R.tile_out(C, k2, d2) + 1
    y, ref = _run_case(ctx, C, k1, d1, k2, d2, L, "bias3", 1.0, False)
    check(_name(precision, C, k1, d1, k2, d2, L, "bias3", 1.0, False), y, ref, R.TOL[precision])
    y, ref = _run_case(ctx, C, k1, d1, k2, d2, L, "spike", 1.0, False)
    check(_name(precision, C, k1, d1, k2, d2, L, "spike", 1.0, False), y, ref, R.TOL[precision])
    (x, w1, b1, w2, b2, _), _ = R.mrf_case(C, k1, d1, k2, d2, L, "spike", 1.0, False)
    zero = ctx.op_mrf_pair(torch.zeros(1, C, L), w1, b1, d1, R.SLOPE, w2, b2, d2, R.SLOPE).cpu()
    assert torch.equal(y[2:3], zero)
    check(_name(precision, C, k1, d1, k2, d2, L, "zero", 1.0, False), zero, ref[2:3], R.TOL[precision])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k,d", R.MRF_SINGLES)
def test_resblock2_step_lengths_and_epilogues(ctxs, k, d, precision):
    """One ResBlock2 step (w2 = None) at C = 64: halo_conv1d_kernel with residual, out_scale and accumulate in bf16x3; (7, 12)
    needs 36 halo rows, past the kernel's 32, and must fall back to the implicit GEMM and still be right."""
    C = 64
    for L in R.mrf_lengths(C):
        for out_scale, acc in R.MRF_EPILOGUES:
            y, ref = _run_case(ctxs[precision], C, k, d, 0, 1, L, "randn", out_scale, acc)
            check(_name(precision, C, k, d, 0, 1, L, "randn", out_scale, acc), y, ref, R.TOL[precision])


def _halo_rows(ctx, run):
    ctx.prof_begin()
    try:
        run()
    finally:
        rows = ctx.prof_end()
    return sorted(n for n in rows if n.startswith("halo_"))


@pytest.mark.parametrize("C", R.MRF_C)
def test_halo_kernels_are_taken_where_the_limits_allow(ctxs, C):
    """The kernel names of the bf16x3 runs above: the fused pair / the halo kernel for C = 32 and 64 inside their limits, neither
    for C = 48, for a reach of 36 rows, or in the f32 mode."""
    L = 70
    for (k1, d1, k2, d2) in R.MRF_PAIRS:
        for precision in PRECISIONS:
            rows = _halo_rows(ctxs[precision], lambda: _run_case(ctxs[precision], C, k1, d1, k2, d2, L, "randn", 1.0, False))
            want = [f"halo_pair_bf16x3<{C}>"] if precision == "bf16x3" and R.halo_pair_covers(C, k1, d1, k2, d2) else []
            assert rows == want, (C, k1, d1, k2, d2, precision, rows)
    for (k, d) in R.MRF_SINGLES:
        rows = _halo_rows(ctxs["bf16x3"], lambda: _run_case(ctxs["bf16x3"], C, k, d, 0, 1, L, "randn", 1.0 / 3.0, True))
        want = [f"halo_conv1d_bf16x3<{C}>"] if R.halo_single_covers(C, k, d) else []
        assert rows == want, (C, k, d, rows)
    assert R.halo_pair_covers(C, 3, 1, 3, 1) == (C != 48)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", R.MRF_C)
def test_halo_switching_is_bit_identical(ctxs, C, precision):
    """MAA_HALO=single (two halo launches) and MAA_HALO=off (implicit GEMM) against the default (fused pair): the three engines
    promise the same products in the same order.  Every tile geometry: all pairs, and as a single step every (k, d) the halo
    kernel covers, at one row, a tile and a one-row tail, two tiles and a one-row tail; B = 3, out_scale = 1/3, accumulate."""
    from audiogpt_amd.backend import reload_tuning
    ctx = ctxs[precision]
    steps = list(R.MRF_PAIRS) + [(k, d, 0, 1) for (k, d) in R.MRF_SINGLES if R.halo_single_covers(C, k, d)]
    cases = [(C, k1, d1, k2, d2, L, "randn", 1.0 / 3.0, True) for (k1, d1, k2, d2) in steps
             for L in (1, R.tile_out(C, k2 or 1, d2) + 1, 2 * R.tile_out(C, k2 or 1, d2) + 1)]
    halo = precision == "bf16x3" and C != 48
    default = {}
    for case in cases:
        default[case], ref = _run_case(ctx, *case)
        check(_name(precision, *case) + "_default", default[case], ref, R.TOL[precision])
    try:
        for mode, rows_want in (("single", [f"halo_conv1d_bf16x3<{C}>"]), ("off", [])):
            os.environ["MAA_HALO"] = mode
            reload_tuning()
            for case in cases:
                got = {}
                rows = _halo_rows(ctx, lambda: got.update(zip(("y", "ref"), _run_case(ctx, *case))))
                check(_name(precision, *case) + "_" + mode, got["y"], got["ref"], R.TOL[precision])
                assert torch.equal(got["y"], default[case]), (mode, case, float((got["y"] - default[case]).abs().max()))
                assert rows == (rows_want if halo else []), (mode, case, rows)
    finally:
        os.environ.pop("MAA_HALO", None)
        reload_tuning()
    for case in cases:
        assert torch.equal(_run_case(ctx, *case)[0], default[case]), case


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", R.MRF_C)
def test_mrf_pair_batch_invariance(ctxs, C, precision):
    """Sample 1 alone equals sample 1 inside B = 3, bit for bit (pair and single step)."""
    ctx = ctxs[precision]
    for (k1, d1, k2, d2) in ((11, 5, 11, 1), (5, 6, 0, 1)):
        L = R.tile_out(C, k2 or 1, d2) + 1
        case = (C, k1, d1, k2, d2, L, "randn", 1.0 / 3.0, True)
        full, _ = _run_case(ctx, *case)
        (x, w1, b1, w2, b2, prev), _ = R.mrf_case(*case)      # (out_prev of the lone sample is sample 1's too)
        one = ctx.op_mrf_pair(x[1:2].contiguous(), w1, b1, d1, R.SLOPE, w2, b2, d2, R.SLOPE, 1.0 / 3.0, prev[1:2].contiguous()).cpu()
        assert torch.equal(one, full[1:2]), (k1, d1, k2, d2, float((one - full[1:2]).abs().max()))


# ------------------------------------------------------------------------------------------------------- transposed conv
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Cin,Cout,k,s,L", R.CONVTR)
def test_conv_transpose1d_shapes(ctxs, Cin, Cout, k, s, L, precision):
    """U = k / s = 1 (one tap, no carry), 2 (the shipped configs: carry groups 0 and 1), 3 (one group, carry 1); L = 1 and 2; odd
    Cin; Cout = 1.  The impulse (one 1 at b = 1, ci = 3, l = L - 1) must give w[3] at the right phase plus bias, and bias
    everywhere else: a phase shift or a dropped tap shows exactly."""
    ctx = ctxs[precision]
    x, w, b = R.convtr_inputs(Cin, Cout, k, s, L)
    for leaky in (0.0, 0.1):
        y = ctx.op_conv_transpose1d(x, w, b, s, leaky=leaky)
        check(f"vocop_convtr_{precision}_{Cin}_{Cout}_k{k}_s{s}_L{L}_leaky{leaky}", y, R.conv_transpose1d_ref(x, w, b, s, leaky),
              R.TOL[precision])
    xi, w, b, want = R.convtr_impulse(Cin, Cout, k, s, L)
    y = ctx.op_conv_transpose1d(xi, w, b, s, leaky=0.1)
    check(f"vocop_convtr_{precision}_{Cin}_{Cout}_k{k}_s{s}_L{L}_impulse", y, want, R.TOL[precision])


def test_conv_transpose1d_refuses_what_the_polyphase_form_does_not_cover(ctxs):
    from audiogpt_amd._lib import MaaError
    for k, s, rule in R.CONVTR_REFUSED:
        x, w, b = R.convtr_inputs(32, 16, k, s, 5)
        with pytest.raises(MaaError, match=rule):
            ctxs["f32"].op_conv_transpose1d(x, w, b, s)
