"""CPU checks of the vocoder operator references (tests/vocoder_ref.py), and the statement that the gates of
tests/test_gpu_vocoder_ops.py can be met: a float64 emulation of the bf16 hi / lo operand split stays within HALF of the
bf16x3 tolerance on every input set the GPU tests use, so a GPU failure is not the inputs' fault."""
import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_ref as R


def test_kaiser_taps_are_the_oracles():
    from oracle import vocoder as O
    f = R.kaiser_sinc12()
    assert f.dtype == torch.float64 and abs(float(f.sum()) - 1.0) < 1e-6
    assert torch.equal(f, f.flip(0))                                   # linear phase
    assert float((f - O.kaiser_sinc_filter1d(0.25, 0.3, 12).double()).abs().max()) < 1e-6


@pytest.mark.parametrize("L", [1, 2, 7, 64, 65])
def test_snake_ref_matches_the_oracle_chain(L):
    from oracle import vocoder as O
    C = 5
    x = torch.randn(2, C, L, generator=R.gen(L))
    al, be = R.snake_params(C)
    filt = O.kaiser_sinc_filter1d(0.25, 0.3, 12).double()
    for logscale in (True, False):
        be_ = be if logscale else be.abs() + 0.5
        want = O.downsample1d(O.snake(O.upsample1d(x.double(), filt), al.double(), be_.double(), logscale), filt)
        assert R.rel_max(R.snake_aa_ref(x, al, be_, logscale), want) < 1e-6
        assert R.rel_max(R.snake_fp32_restatement(x, al, be_, logscale), want) < 1e-5


def test_snake_spike_input_shows_a_wrong_clamp():
    """Reflecting instead of replicating at the ends, or reading one row off, is far outside the tolerance on the spike input."""
    C, L = 4, 65
    x = R.snake_input(C, L, "spike")
    al, be = R.snake_params(C)
    ref = R.snake_aa_ref(x, al, be, True)
    assert R.rel_max(R.snake_aa_ref(x.roll(1, 2), al, be, True), ref) > 100 * R.SNAKE_TOL
    shifted = x.clone()
    shifted[:, :, 63], shifted[:, :, 64] = x[:, :, 62], x[:, :, 63]     # tile 1 staged from one row too low
    assert R.rel_max(R.snake_aa_ref(shifted, al, be, True), ref) > 100 * R.SNAKE_TOL


def test_mrf_pair_ref_matches_two_conv1d_modules():
    C, L = 6, 40
    for (k1, d1, k2, d2) in R.MRF_PAIRS:
        x, w1, b1, w2, b2, prev = R.mrf_inputs(C, k1, d1, k2, d2, L)
        c1 = torch.nn.Conv1d(C, C, k1, 1, dilation=d1, padding=(k1 * d1 - d1) // 2).double()
        c2 = torch.nn.Conv1d(C, C, k2, 1, dilation=d2, padding=(k2 * d2 - d2) // 2).double()
        with torch.no_grad():
            c1.weight.copy_(w1), c1.bias.copy_(b1), c2.weight.copy_(w2), c2.bias.copy_(b2)
            xd = x.double()
            xt = c1(F.leaky_relu(xd, 0.1))                              # ResBlock1's inner step
            xt = c2(F.leaky_relu(xt, 0.1))
            step = xt + xd
            single = c1(F.leaky_relu(xd, 0.1)) + xd                     # ResBlock2's
        assert R.rel_max(R.mrf_pair_ref(x, w1, b1, k1, d1, 0.1, w2, b2, k2, d2, 0.1, 1.0, None), step) < 1e-12
        assert R.rel_max(R.mrf_pair_ref(x, w1, b1, k1, d1, 0.1, w2, b2, k2, d2, 0.1, 1 / 3, prev), prev.double() + step / 3) < 1e-12
        assert R.rel_max(R.mrf_pair_ref(x, w1, b1, k1, d1, 0.1, None, None, 0, 1, 0.1, 0.5, prev), prev.double() + single / 2) < 1e-12
        assert R.mrf_pair_ref(x, w1, b1, k1, d1, 0.1, w2, b2, k2, d2, 0.1, 1.0, None).shape == x.shape


def test_shape_lists_reach_every_path():
    assert R.mrf_lengths(32, 11, 1)[-1] == 493 and R.mrf_lengths(32, 3, 1)[-1] == 509     # the largest case is 3 x 32 x 509
    assert R.mrf_lengths(64, 7, 1) == (1, 2, 121, 122, 123, 245)
    assert all(R.halo_pair_covers(C, *p) for C in (32, 64) for p in R.MRF_PAIRS) and not R.halo_pair_covers(48, 3, 1, 3, 1)
    assert [R.halo_single_covers(64, k, d) for k, d in R.MRF_SINGLES] == [True, True, False]
    U = sorted({k // s for _, _, k, s, _ in R.CONVTR})
    assert U == [1, 2, 3]
    for _, _, k, s, _ in R.CONVTR:                                      # what the library accepts
        assert k % s == 0 and (k - s) % 2 == 0 and (s - 1 + (k - s) // 2) // s <= 1
    for k, s, _ in R.CONVTR_REFUSED:
        assert k % s != 0 or (k - s) % 2 != 0 or (s - 1 + (k - s) // 2) // s > 1


def _bias3_shows_a_wrong_intermediate(C, k1, d1, k2, d2):
    """c2 fed c1(0) + b1 outside [0, L) instead of zeros: the edge outputs move by O(1)."""
    L = R.tile_out(C, k2, d2) + 1
    x, w1, b1, w2, b2, _ = R.mrf_inputs(C, k1, d1, k2, d2, L, "bias3")
    ref = R.mrf_pair_ref(x, w1, b1, k1, d1, 0.1, w2, b2, k2, d2, 0.1, 1.0, None)
    h2 = d2 * (k2 - 1) // 2
    xp = F.pad(x.double(), (h2, h2))                                     # c1 evaluated h2 positions past each end
    t = F.conv1d(F.leaky_relu(xp, 0.1), w1.double(), b1.double(), padding=d1 * (k1 - 1) // 2, dilation=d1)
    wrong = F.conv1d(F.leaky_relu(t, 0.1), w2.double(), b2.double(), dilation=d2) + x.double()
    assert wrong.shape == ref.shape
    d = (wrong - ref).abs()
    assert float(d[:, :, :h2].max()) > 0.3 and float(d[:, :, -h2:].max()) > 0.3
    assert float(d[:, :, h2:L - h2].max()) < 1e-12


@pytest.mark.parametrize("C", R.MRF_C)
def test_mrf_inputs_the_bf16_split_meets_the_gate(C):
    gate = 0.5 * R.TOL["bf16x3"]
    for (k1, d1, k2, d2) in R.MRF_PAIRS:
        _bias3_shows_a_wrong_intermediate(C, k1, d1, k2, d2)
        cases = [(L, "randn") for L in R.mrf_lengths(C, k2, d2)]
        cases += [(R.tile_out(C, k2, d2) + 1, "bias3"), (R.tile_out(C, k2, d2) + 1, "spike")]
        for L, kind in cases:
            x, w1, b1, w2, b2, prev = R.mrf_inputs(C, k1, d1, k2, d2, L, kind)
            for out_scale, acc in (R.MRF_EPILOGUES if kind == "randn" else R.MRF_EPILOGUES[:1]):
                args = (x, w1, b1, k1, d1, 0.1, w2, b2, k2, d2, 0.1, out_scale, prev if acc else None)
                e = R.rel_max(R.mrf_pair_emulated(*args), R.mrf_pair_ref(*args))
                assert e <= gate, (C, k1, d1, k2, d2, L, kind, out_scale, acc, e)


def test_single_conv_inputs_the_bf16_split_meets_the_gate():
    C = 64
    for k, d in R.MRF_SINGLES:
        for L in R.mrf_lengths(C):
            x, w1, b1, _, _, prev = R.mrf_inputs(C, k, d, 0, 1, L)
            for out_scale, acc in R.MRF_EPILOGUES:
                args = (x, w1, b1, k, d, 0.1, None, None, 0, 1, 0.1, out_scale, prev if acc else None)
                e = R.rel_max(R.mrf_pair_emulated(*args), R.mrf_pair_ref(*args))
                assert e <= 0.5 * R.TOL["bf16x3"], (k, d, L, out_scale, acc, e)


@pytest.mark.parametrize("shape", R.CONVTR)
def test_convtr_inputs_the_bf16_split_meets_the_gate_and_the_impulse_is_the_kernel(shape):
    x, w, b = R.convtr_inputs(*shape)
    s = shape[3]
    for leaky in (0.0, 0.1):
        ref = R.conv_transpose1d_ref(x, w, b, s, leaky)
        assert ref.shape == (R.B, shape[1], shape[4] * s)
        assert R.rel_max(R.convtr_emulated(x, w, b, s, leaky), ref) <= 0.5 * R.TOL["bf16x3"]
    xi, w, b, want = R.convtr_impulse(*shape)
    assert R.rel_max(R.conv_transpose1d_ref(xi, w, b, s, 0.1), want) < 1e-12
    assert R.rel_max(R.convtr_emulated(xi, w, b, s, 0.1), want) <= 0.5 * R.TOL["bf16x3"]
