"""The waveform front ends on the device, each against a float64 reference on the CPU (tests/frontend_ref.py): the small kernels
of csrc/spectral.hip alone (through maa_op_front_rows, which forwards every argument of the library's internal launches, and
maa_clap_similarity), the Spectral handle (pad -> framed DFT with overlapping A rows -> power -> mel product -> logarithm) at
small transforms, every setting, hop below, at and above n_fft, signals down to one sample and batches whose rows differ, the
Resampler handle at six ratios whose row pitches take both A gathers of the contraction (orig = 160 / 441 / 3 / 1, banks of 441 / 160 / 1 / 2 / 3 / 147 phases), and
DeviceMelTransform.resample against the scalar resampy loop of the oracle, carry outputs and zeroed tail included.

The context runs in "bf16x3": the front ends must run in exact fp32 whatever the context says.  Every output is written into a
buffer pre-filled with a sentinel that has 64 spare floats behind it: a column that should have been written as zero shows up,
and so does a store past the end, with every access still inside an allocation.

Gates (tests/frontend_ref.py states them; tests/test_frontend_ref.py shows on the CPU that float32 numpy stays within half of each
on every input used here): pad bit-equal; power 1e-6 relative per element; log-mel 1e-4 dB / 1e-6 absolute; the bn0 affine 1e-6
and the reductions (pool, similarity) 2e-5 of their scale; the resamplers 1e-5 rel-max; Spectral per element the 2e-5 reduction
gate on the linear mel, relative to the largest mel of its frame, carried through the logarithm, plus the logarithm's gate.

Findings that are not bugs:
  * power, the planted denormal pair (re^2 + im^2 below the smallest normal float32): float32 cannot hold the sum to a relative
    gate there -- numpy's own float32 evaluation gives 0 where float64 gives 1e-40 -- so the elements whose exact sum of squares is
    below FLT_MIN, the planted pair alone, are held to an absolute FLT_MIN (power 2) or sqrt(FLT_MIN) (power 1); every other
    element, the denormal beside 1 included, is held to the relative gate.
  * Spectral, the floor: an element is compared exactly only where the reference's linear mel is at or below amin; the inputs keep
    every other element above 1.001 amin (tests/test_frontend_ref.py), so the exact comparison applies to the silent row alone."""
import math

import numpy as np
import pytest
import torch

from tests import frontend_ref as R
from tests.util import check, record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
PAD = 64                 # spare floats behind every output


@pytest.fixture(scope="module")
def ctx():
    from audiogpt_amd.backend import Context
    c = Context(DEV, precision="bf16x3")
    yield c
    c.close()


@pytest.fixture(scope="module")
def dmt(ctx):
    from audiogpt_amd.mel import DeviceMelTransform
    return DeviceMelTransform(ctx)


def guarded(numel):
    """A device buffer of numel + PAD floats, all of it the sentinel."""
    return torch.full((numel + PAD,), SENTINEL, dtype=torch.float32, device=DEV)


def taken(buf, shape):
    """The front of the buffer on the CPU as a numpy array of `shape`, after checking that the sentinel behind it did not move."""
    t = buf.cpu().numpy()
    numel = int(np.prod(shape))
    assert bool((t[numel:] == SENTINEL).all()), "store past the end of the output"
    return t[:numel].reshape(shape)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------- pad

def run_pad(ctx, x, left, right, mode, ldo):
    B, n = x.shape
    out = guarded(B * ldo)
    ctx.op_front_rows("pad", dev(x), out, B=B, n=n, left=left, total=left + n + right, ldo=ldo, mode=mode)
    return taken(out, (B, ldo))


@pytest.mark.parametrize("n,left,right", R.PAD_CASES)
@pytest.mark.parametrize("B", R.PAD_B)
def test_pad(ctx, B, n, left, right):
    total = n + left + right
    x = R.wave(B, n, n + B)
    for mode, name in enumerate(("constant", "reflect")):
        if name == "reflect" and (n <= left or n <= right):
            continue
        for ldo in (total, (total + 3) // 4 * 4 + 4):
            got = run_pad(ctx, x, left, right, mode, ldo)
            assert np.array_equal(bits(got), bits(R.pad_ref(x, left, right, name, ldo))), (name, ldo)


@pytest.mark.parametrize("n,left,right", R.PAD_REFUSED)
def test_pad_refuses_a_reflection_as_long_as_the_signal(ctx, n, left, right):
    from audiogpt_amd._lib import MaaError
    x = R.wave(2, n, 5)
    with pytest.raises(MaaError, match="reflect padding needs a signal longer than the pad"):
        run_pad(ctx, x, left, right, 1, n + left + right)
    x = R.wave(2, n + 1, 6)          # one sample more is taken, by the same context
    got = run_pad(ctx, x, left, right, 1, n + 1 + left + right)
    assert np.array_equal(bits(got), bits(R.pad_ref(x, left, right, "reflect", n + 1 + left + right)))


# ---------------------------------------------------------------------------------------------------- power

@pytest.mark.parametrize("nf", R.POWER_NF)
@pytest.mark.parametrize("rows", R.POWER_ROWS)
def test_power(ctx, rows, nf):
    for ldm, ldy in (((nf + 3) // 4 * 4, 2 * nf), (nf + 7, 2 * nf + 1)):
        y = R.power_input(rows, nf, ldy, rows + nf)
        under = np.zeros((rows, ldm), bool)
        under[:, :nf] = (y[:, :nf].astype(np.float64) ** 2 + y[:, nf:2 * nf].astype(np.float64) ** 2) < R.FLT_MIN
        for power2 in (0, 1):
            out = guarded(rows * ldm)
            ctx.op_front_rows("power", dev(y), out, rows=rows, nf=nf, ldy=ldy, ldm=ldm, power2=power2)
            got = taken(out, (rows, ldm))
            ref = R.power_ref(y, nf, ldm, power2)
            assert np.isfinite(got).all()
            assert not bits(got[:, nf:]).any(), "columns nf .. ldm-1 are not +0"
            assert not got[ref == 0].any()
            err = np.abs(got - ref)
            rel = float((err[~under & (ref > 0)] / ref[~under & (ref > 0)]).max())
            record("front_power_r%d_nf%d_ldm%d_p%d" % (rows, nf, ldm, 2 if power2 else 1), rel_max=rel, tol=R.TOL_POWER)
            assert rel <= R.TOL_POWER, (ldm, power2, rel)
            assert bool((err[under] <= R.TOL_POWER * ref[under] + R.power_floor(power2)).all())


# ---------------------------------------------------------------------------------------------------- log-mel

@pytest.mark.parametrize("kind,amin", R.LOGMEL_KINDS)
@pytest.mark.parametrize("n_mels", R.LOGMEL_MELS)
def test_logmel(ctx, n_mels, kind, amin):
    tol = R.TOL_DB if kind == 0 else R.TOL_T16K
    worst = 0.0
    for B in R.LOGMEL_B:
        for frames in R.LOGMEL_FRAMES:
            for ldmel in (n_mels, n_mels + 3):
                x = R.logmel_input(B, frames, n_mels, ldmel, kind, amin, n_mels + frames)
                xd = dev(x)
                low = x[:, :n_mels].reshape(B, frames, n_mels) <= np.float32(amin)
                for layout in (0, 1):
                    out = guarded(B * frames * n_mels)
                    ctx.op_front_rows("logmel", xd, out, B=B, frames=frames, n_mels=n_mels, ldmel=ldmel, log_kind=kind, amin=amin,
                                      ref_db=0.0, layout=layout)
                    ref = R.logmel_ref(x, B, frames, n_mels, kind, amin, 0.0, layout)
                    got = taken(out, ref.shape)
                    assert np.isfinite(got).all()
                    worst = max(worst, float(np.abs(got - ref).max()))
                    assert float(np.abs(got - ref).max()) <= tol, (B, frames, ldmel, layout, float(np.abs(got - ref).max()))
                    floor = got[low if layout == 0 else low.transpose(0, 2, 1)]
                    assert floor.size >= 4 and len(set(bits(floor).tolist())) == 1, "inputs at or below amin give more than one value"
                    if kind == 1:
                        pre = R.logmel_ref(x, B, frames, n_mels, kind, amin, 0.0, layout, clip=False)
                        assert not bits(got[pre < 0]).any() and bool((got[pre > 1] == 1.0).all()), "a clipped value is not exactly 0 or 1"
    record("front_logmel_m%d_k%d" % (n_mels, kind), abs_max=worst, tol=tol)


# ---------------------------------------------------------------------------------------------------- bn0 affine, Cnn14 pooling

@pytest.mark.parametrize("rows,F", R.AFFINE_SHAPES)
def test_affine(ctx, rows, F):
    x, scale, shift = R.affine_input(rows, F, rows)
    out = guarded(rows * F)
    ctx.op_front_rows("affine", dev(x), out, scale=torch.from_numpy(scale), shift=torch.from_numpy(shift), n=rows * F, F=F)
    check("front_affine_r%d_F%d" % (rows, F), taken(out, (rows * F,)), R.affine_ref(x, F, scale, shift), R.TOL_AFFINE)


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_pool(ctx, shape):
    B, T, F, C = shape
    x = R.pool_input(B, T, F, C, seed=sum(shape))
    out = guarded(B * C)
    ctx.op_front_rows("pool", dev(x), out, B=B, T=T, F=F, C=C)
    got, ref = taken(out, (B, C)), R.pool_ref(x)
    check("front_pool_%dx%dx%dx%d" % shape, got, ref, R.TOL_REDUCE)
    # by channel too: the negative channel (a maximum that comes from the data, not from its seed), the constant one, the offset one
    for c in (1, 2, 3):
        check("front_pool_%dx%dx%dx%d_c%d" % (shape + (c,)), got[:, c], ref[:, c], R.TOL_REDUCE)


# ---------------------------------------------------------------------------------------------------- similarity

@pytest.mark.parametrize("D", R.SIM_D)
def test_similarity(ctx, D):
    worst = 0.0
    for Na in R.SIM_NA:
        for Nt in R.SIM_NT:
            a, t = R.similarity_input(Na, Nt, D, D + Na + Nt)
            ad, td = dev(a), dev(t)
            for scale in R.SIM_SCALE:
                out = guarded(Na * Nt)
                ctx._call("maa_clap_similarity", ad.data_ptr(), td.data_ptr(), Na, Nt, D, float(scale), out.data_ptr())
                got, ref = taken(out, (Na, Nt)), R.similarity_ref(a, t, scale)
                bound = scale * float(np.outer(np.linalg.norm(a.astype(np.float64), axis=1),
                                               np.linalg.norm(t.astype(np.float64), axis=1)).max())
                r = float(np.abs(got - ref).max()) / bound
                worst = max(worst, r)
                assert np.isfinite(got).all() and r <= R.TOL_REDUCE, (Na, Nt, scale, r)
    record("front_similarity_D%d" % D, rel_max=worst, tol=R.TOL_REDUCE)


# ---------------------------------------------------------------------------------------------------- Spectral

def make_spectral(ctx, config, cfg):
    from audiogpt_amd.backend import Spectral
    basis, melw = R.spectral_tables(config)
    return Spectral(ctx, cfg, basis, melw)


def run_spectral(sp, x):
    B, n = x.shape
    T, M = sp.frames(n), sp.cfg["n_mels"]
    out = guarded(B * T * M)
    sp._call("maa_spectral_forward", dev(x).data_ptr(), B, n, out.data_ptr())
    return taken(out, (B, T, M) if sp.cfg["out_layout"] == "btm" else (B, M, T))


def spectral_worst(got, x, cfg, config):
    """(max |got - ref| / gate over the elements, after the floor check; the reference's linear mel; rel-max of the output)."""
    ref, mel = R.spectral_ref(x, cfg, *R.spectral_tables(config))
    assert got.shape == ref.shape and np.isfinite(got).all()
    R.check_floor(got, mel, cfg)
    return float((np.abs(got - ref) / R.spectral_gate(mel, cfg)).max()), mel, R.rel_max(got, ref)


@pytest.mark.parametrize("config", R.SPECTRAL_CONFIGS)
def test_spectral(ctx, config):
    n_fft, hop, n_mels = config
    for case in [c for c in R.spectral_cases() if c[0] == config]:
        cfg = R.spectral_cfg(*case[:5])
        sp = make_spectral(ctx, config, cfg)
        worst = rel = 0.0
        for n in R.spectral_lengths(n_fft, hop, cfg["pad_mode"]):
            x = R.spectral_input(case, n)
            w, _, r = spectral_worst(run_spectral(sp, x), x, cfg, config)
            worst, rel = max(worst, w), max(rel, r)
            assert w <= 1.0, "%s n=%d: %.3f of the per-element gate" % (case, n, w)
        record("front_spectral_%d_%d_%d_%s_p%d_%s_%s_B%d" % (config + case[1:]), rel_max=rel, gate_fraction=worst, tol=1.0)
        sp.close()


@pytest.mark.parametrize("log_kind", ("db", "transforms_16000"))
def test_spectral_silent_row(ctx, log_kind):
    cfg, x = R.silent_case(log_kind)
    sp = make_spectral(ctx, R.SILENT_CONFIG, cfg)
    got = run_spectral(sp, x)
    w, mel, _ = spectral_worst(got, x, cfg, R.SILENT_CONFIG)
    assert w <= 1.0, w
    assert R.check_floor(got[1:2], mel[1:2], cfg) == got[1].size          # the whole silent row, one value
    for b in (0, 2):          # the rows beside it are what they are alone
        assert np.array_equal(bits(run_spectral(sp, x[b:b + 1])[0]), bits(got[b])), b
    sp.close()


def test_spectral_loud_row_clips_to_one(ctx):
    cfg, x = R.loud_case()
    sp = make_spectral(ctx, R.SILENT_CONFIG, cfg)
    got = run_spectral(sp, x)
    assert bool((got == 1.0).all()), float(got.min())
    sp.close()


def test_spectral_refuses_the_shortest_reflection_and_goes_on(ctx):
    from audiogpt_amd._lib import MaaError
    config = R.SPECTRAL_CONFIGS[0]
    n_fft = config[0]
    cfg = R.spectral_cfg(config, "reflect", 2, "db", "btm")
    sp = make_spectral(ctx, config, cfg)
    with pytest.raises(MaaError, match="signal too short for reflect padding"):
        run_spectral(sp, R.wave(2, n_fft // 2, 3))
    x = R.wave(2, n_fft // 2 + 1, 4)
    w, _, _ = spectral_worst(run_spectral(sp, x), x, cfg, config)
    assert w <= 1.0, w
    sp.close()


# ---------------------------------------------------------------------------------------------------- Resampler

def run_resampler(rs, x):
    B, n = x.shape
    target = -(-rs.new * n // rs.orig)
    out = guarded(B * target)
    rs._call("maa_resampler_forward", dev(x).data_ptr(), B, n, out.data_ptr())
    return taken(out, (B, target))


@pytest.mark.parametrize("ratio,reduced", list(zip(R.RESAMPLE_RATIOS, R.RESAMPLE_REDUCED)))
def test_resampler(ctx, ratio, reduced):
    from audiogpt_amd.backend import Resampler
    orig, new = reduced
    bank, width = R.sinc_bank(*ratio)
    rs = Resampler(ctx, orig, new, width, bank)
    for n in R.resample_lengths(orig):
        for B in R.RESAMPLE_B:
            x = R.wave(B, n, 7 * n + B)
            ref = R.resample_ref(x, bank, width, orig, new)
            assert ref.shape == (B, math.ceil(new * n / orig))
            check("front_resample_%d_%d_n%d_B%d" % (orig, new, n, B), run_resampler(rs, x), ref, R.TOL_RESAMPLE)
    # placement, without the float64 reference: a unit impulse at sample s puts bank[p, width + s - q orig] at output q new + p
    n = 2 * orig + 3
    x = np.zeros((2, n), np.float32)
    x[0, 0] = x[1, n - 1] = 1.0
    got = run_resampler(rs, x)
    q, p = np.divmod(np.arange(got.shape[1]), new)
    for b, s in ((0, 0), (1, n - 1)):
        col = width + s - q * orig
        want = np.where((col >= 0) & (col < bank.shape[1]), bank[p, np.clip(col, 0, bank.shape[1] - 1)], 0.0)
        assert np.count_nonzero(want) >= 3
        assert float(np.abs(got[b] - want).max()) <= R.TOL_PLACE, (b, float(np.abs(got[b] - want).max()))
    rs.close()


# ---------------------------------------------------------------------------------------------------- DeviceMelTransform.resample

@pytest.mark.parametrize("sr", R.DMT_SR)
def test_device_mel_transform_resamples_like_the_scalar_loop(ctx, dmt, sr):
    from audiogpt_amd import mel
    ratio = float(R.DMT_TARGET) / float(sr)
    if sr in R.DMT_CARRY_SR:          # first the outputs of the one-phase carry pass by themselves: a run that skipped it fails here
        n = R.dmt_lengths(sr)[0]
        x, ref = R.dmt_case(sr, n)
        t = mel.resampy_carries(int(n * ratio), sr, R.DMT_TARGET)
        assert t.size >= 1
        got = dmt.resample(dev(x), sr).cpu().numpy()
        check("front_dmt_resample_%d_carries" % sr, got[t], ref[t], R.TOL_RESAMPLE)
    for n in R.dmt_lengths(sr):
        x, ref = R.dmt_case(sr, n)
        got = dmt.resample(dev(x), sr).cpu().numpy()
        assert got.shape == ref.shape == (int(np.ceil(n * ratio)),)
        check("front_dmt_resample_%d_n%d" % (sr, n), got, ref, R.TOL_RESAMPLE)
        if int(n * ratio) < int(np.ceil(n * ratio)):
            assert got[-1] == 0.0

def test_device_mel_transform_leaves_16k_alone(dmt):
    x = dev(R.wave(1, 100, 9)[0])
    assert dmt.resample(x, R.DMT_TARGET) is x
