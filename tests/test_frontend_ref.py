"""tests/frontend_ref.py on the CPU, no library: what gives the gates of tests/test_gpu_frontend_ops.py their meaning.  The framed
DFT of spectral_ref is numpy's rfft of the Hann-windowed frames; resample_ref is the torchaudio restatement of the oracle with the
sinc bank and the scalar resampy loop of the oracle with the resampy bank, its carries and its zeroed tail; for every input the GPU
file uses, the same operation in float32 on the CPU stays within HALF of the gate the GPU file applies; and the inputs meet the
conditions the GPU file's exact comparisons rely on."""
import math

import numpy as np
import pytest
import torch

from tests import frontend_ref as R

F32, F64 = np.float32, np.float64


def half(got, ref, tol, what):
    r = R.rel_max(got, ref)
    assert r <= tol / 2, "%s: float32 on the CPU is %.3e from float64, more than half of %.1e" % (what, r, tol)
    return r


# ---- the references against independent statements of the same operation

@pytest.mark.parametrize("config", R.SPECTRAL_CONFIGS)
def test_framed_dft_is_rfft_of_the_windowed_frames(config):
    from scipy.signal import get_window
    n_fft, hop, n_mels = config
    basis, melw = R.spectral_tables(config)
    assert basis.dtype == F32 and basis.shape == (2 * (n_fft // 2 + 1), n_fft)
    assert melw.shape == (n_mels, n_fft // 2 + 1) and bool((melw.sum(axis=1) > 0).all()), "an empty mel filter"
    win = get_window("hann", n_fft, fftbins=True).astype(F64)          # periodic
    for pad_mode in ("reflect", "constant"):
        for n in R.spectral_lengths(n_fft, hop, pad_mode):
            x = R.wave(3, n, n_fft + n)
            xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode=pad_mode).astype(F64)
            fr = R.frames_of(xp, 1 + n // hop, n_fft, hop)
            assert fr.shape == (3, 1 + n // hop, n_fft) and fr[0, -1, -1] == xp[0, (n // hop) * hop + n_fft - 1]
            y = fr @ basis.astype(F64).T
            z = np.fft.rfft(fr * win, axis=-1)
            want = np.concatenate([z.real, z.imag], axis=-1)
            bound = 1e-6 * np.abs(z).max(axis=-1, keepdims=True)
            assert bool((np.abs(y - want) <= bound).all()), (config, pad_mode, n, float((np.abs(y - want) / bound).max()))


@pytest.mark.parametrize("ratio,reduced,shape", list(zip(R.RESAMPLE_RATIOS, R.RESAMPLE_REDUCED, R.RESAMPLE_BANKS)))
def test_resample_ref_is_the_oracles_torchaudio_resample(ratio, reduced, shape):
    from oracle import clap_audio as O
    bank, width = R.sinc_bank(*ratio)
    orig, new = reduced
    g = math.gcd(*ratio)
    assert (ratio[0] // g, ratio[1] // g) == reduced and bank.shape == shape == (new, 2 * width + orig) and bank.dtype == F32
    for n in R.resample_lengths(orig):
        for B in R.RESAMPLE_B:
            x = R.wave(B, n, 7 * n + B)
            ref = R.resample_ref(x, bank, width, orig, new)
            want = O.resample(torch.from_numpy(x), *ratio).numpy()
            assert ref.shape == want.shape == (B, -(-new * n // orig))
            assert R.rel_max(ref, want) <= 1e-6, (ratio, n, B, R.rel_max(ref, want))
            half(R.resample_ref(x, bank, width, orig, new, F32), ref, R.TOL_RESAMPLE, "resampler %s n=%d" % (ratio, n))


@pytest.mark.parametrize("sr", R.DMT_SR)
def test_resampy_ref_is_the_scalar_loop(sr):
    from audiogpt_amd import mel
    ratio = float(R.DMT_TARGET) / float(sr)
    for n in R.dmt_lengths(sr):
        x, want = R.dmt_case(sr, n)
        ref = R.resampy_ref(x, sr)
        assert ref.shape == want.shape == (int(np.ceil(n * ratio)),)
        assert R.rel_max(ref, want) <= 2e-6, (sr, n, R.rel_max(ref, want))
        half(R.resampy_ref(x, sr, F32), want, R.TOL_RESAMPLE, "resampy %d n=%d" % (sr, n))
        if int(n * ratio) < int(np.ceil(n * ratio)):
            assert want[-1] == 0 and ref[-1] == 0
        # the host restatement the tools use is the same contraction in float32
        half(mel.librosa_resample(x, sr, R.DMT_TARGET), want, R.TOL_RESAMPLE, "mel.librosa_resample %d n=%d" % (sr, n))
    if sr in R.DMT_CARRY_SR:          # what the GPU file's carry assertion relies on
        n = R.dmt_lengths(sr)[0]
        x, want = R.dmt_case(sr, n)
        t = mel.resampy_carries(int(n * ratio), sr, R.DMT_TARGET)
        assert t.size >= 1 and int(t.max()) < int(n * ratio)
        assert int(n * ratio) < int(np.ceil(n * ratio))
        half(R.resampy_ref(x, sr, F32)[t], want[t], R.TOL_RESAMPLE, "resampy carries %d" % sr)
        # without the carry kernel those outputs miss the gate: the assertion can tell
        bank, width = mel.resampy_kernel_bank(sr, R.DMT_TARGET)
        g = math.gcd(sr, R.DMT_TARGET)
        periodic = R.resample_ref(x[None], bank, width, sr // g, R.DMT_TARGET // g)[0]
        assert R.rel_max(periodic[t], want[t]) > R.TOL_RESAMPLE
    else:
        assert mel.resampy_carries(int(3000 * ratio), sr, R.DMT_TARGET).size == 0


# ---- the float32 restatement of every kernel-alone input

def test_pad_inputs():
    for n, left, right in R.PAD_CASES:
        for mode in ("constant", "reflect"):
            if mode == "reflect" and (n <= left or n <= right):
                assert (n, left, right) == (1, 6, 9)
                continue
            total = n + left + right
            for ldo in (total, (total + 3) // 4 * 4 + 4):
                x = R.wave(3, n, n)
                ref = R.pad_ref(x, left, right, mode, ldo)
                assert ref.shape == (3, ldo) and ref.dtype == F32 and bool((ref[:, total:] == 0).all())
                assert np.array_equal(ref[:, left:left + n], x)
                if mode == "reflect" and left:
                    assert np.array_equal(ref[:, left - 1], x[:, 1]) and np.array_equal(ref[:, 0], x[:, left])
                if mode == "reflect":
                    assert np.array_equal(ref[:, left + n], x[:, n - 2])
    assert any(left != right for _, left, right in R.PAD_CASES)
    assert [(n == left, n == right) for n, left, right in R.PAD_REFUSED] == [(True, False), (False, True)]


@pytest.mark.parametrize("nf", R.POWER_NF)
@pytest.mark.parametrize("rows", R.POWER_ROWS)
def test_power_fp32_within_half(rows, nf):
    for ldm, ldy in (((nf + 3) // 4 * 4, 2 * nf), (nf + 7, 2 * nf + 1)):
        y = R.power_input(rows, nf, ldy, rows + nf)
        assert float(np.abs(y).max()) <= 1.0001e15 and y[0, 0] == 0 and y[0, nf] == 0
        assert 0 < abs(float(y[0, 1])) < R.FLT_MIN and 0 < abs(float(y[0, nf + 1])) < R.FLT_MIN          # the denormal pair
        for power2 in (0, 1):
            ref = R.power_ref(y, nf, ldm, power2)
            got = R.power_ref(y, nf, ldm, power2, F32)
            assert np.isfinite(got).all() and ref[0, 0] == 0 and bool((ref[:, nf:] == 0).all())
            assert bool((np.abs(got - ref) <= R.TOL_POWER / 2 * np.abs(ref) + R.power_floor(power2)).all())
            # the floor is used by the planted denormal pair alone
            under = (y[:, :nf].astype(F64) ** 2 + y[:, nf:2 * nf].astype(F64) ** 2) < R.FLT_MIN
            assert int(under.sum()) == 2 and under[0, 0] and under[0, 1]
            assert bool((np.abs(got - ref)[:, :nf][~under] <= R.TOL_POWER / 2 * np.abs(ref)[:, :nf][~under]).all())


@pytest.mark.parametrize("kind,amin", R.LOGMEL_KINDS)
@pytest.mark.parametrize("n_mels", R.LOGMEL_MELS)
def test_logmel_fp32_within_half(n_mels, kind, amin):
    tol = R.TOL_DB if kind == 0 else R.TOL_T16K
    for B in R.LOGMEL_B:
        for frames in R.LOGMEL_FRAMES:
            for ldmel in (n_mels, n_mels + 3):
                x = R.logmel_input(B, frames, n_mels, ldmel, kind, amin, n_mels + frames)
                assert x[0, 0] == F32(amin) and 0 < x[0, 1] < F32(amin) and x[0, 3] == 0
                assert bool((x[:, n_mels:] == R.LOGMEL_PAD_VALUE).all())
                for layout in (0, 1):
                    ref = R.logmel_ref(x, B, frames, n_mels, kind, amin, 0.0, layout)
                    got = R.logmel_ref(x, B, frames, n_mels, kind, amin, 0.0, layout, F32)
                    assert ref.shape == ((B, frames, n_mels) if layout == 0 else (B, n_mels, frames))
                    assert float(np.abs(got - ref).max()) <= tol / 2, (n_mels, kind, float(np.abs(got - ref).max()))
                at_floor =R.logmel_ref(x, B, frames, n_mels, kind, amin, 0.0, 0, F32)[x[:, :n_mels].reshape(B, frames, n_mels) <= F32(amin)]
                assert at_floor.size >= 4 and bool((at_floor == at_floor[0]).all())
                if kind == 1:          # the exact 0.0 / 1.0 of the clip: no input within ten gates of either threshold
                    pre = R.logmel_ref(x, B, frames, n_mels, kind, amin, 0.0, 0, clip=False)
                    assert float(np.minimum(np.abs(pre), np.abs(pre - 1)).min()) > 10 * tol
                    assert bool((pre < 0).sum() >= 5) and bool((pre > 1).sum() >= 2) and pre.reshape(-1)[4] < 0 < 1 < pre.reshape(-1)[5]


@pytest.mark.parametrize("rows,F", R.AFFINE_SHAPES)
def test_affine_fp32_within_half(rows, F):
    x, scale, shift = R.affine_input(rows, F, rows)
    half(R.affine_ref(x, F, scale, shift, F32), R.affine_ref(x, F, scale, shift), R.TOL_AFFINE, "affine")


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_pool_fp32_within_half(shape):
    x = R.pool_input(*shape, seed=sum(shape))
    ref = R.pool_ref(x)
    half(R.pool_ref(x, F32), ref, R.TOL_REDUCE, "pool")
    assert bool((x[..., 1] < 0).all()) and bool((ref[:, 1] < -0.5).all())          # a maximum seeded with 0 would give > -0.5 there
    assert bool((x[..., 2] == x[0, 0, 0, 2]).all()) and bool((x[..., 3] > 990).all())
    assert bool((np.delete(x, 1, axis=-1) >= 0).all())


@pytest.mark.parametrize("D", R.SIM_D)
def test_similarity_fp32_within_half(D):
    for Na in R.SIM_NA:
        for Nt in R.SIM_NT:
            a, t = R.similarity_input(Na, Nt, D, D + Na + Nt)
            for scale in R.SIM_SCALE:
                ref = R.similarity_ref(a, t, scale)
                bound = scale * float(np.outer(np.linalg.norm(a.astype(F64), axis=1), np.linalg.norm(t.astype(F64), axis=1)).max())
                assert float(np.abs(R.similarity_ref(a, t, F32(scale), F32) - ref).max()) <= R.TOL_REDUCE / 2 * bound
                if D >= 2:
                    assert ref[0, 0] == 0 and np.linalg.norm(a[0]) > 0 and np.linalg.norm(t[0]) > 0          # the orthogonal pair
            norms = np.linalg.norm(a, axis=1)
            assert Na == 1 or float(norms.max() / norms.min()) > 1.5 or D == 1


# ---- the handles' inputs

def test_the_spectral_cases_cover_every_setting_with_every_n_fft():
    cases = R.spectral_cases()
    assert len(cases) == 24 and len(set(cases)) == 24
    for n_fft in sorted({c[0] for c in R.SPECTRAL_CONFIGS}):
        mine = [c for c in cases if c[0][0] == n_fft]
        for pos, values in ((1, ("reflect", "constant")), (2, (1, 2)), (3, ("db", "transforms_16000")), (4, ("btm", "bmt")), (5, (1, 3))):
            assert {c[pos] for c in mine} == set(values), (n_fft, pos)
    assert {(c[2], c[4]) for c in cases} == {(1, "btm"), (1, "bmt"), (2, "btm"), (2, "bmt")}
    hops = {(c[1] >= c[0]) for c in R.SPECTRAL_CONFIGS}
    assert hops == {False, True} and any(c[1] > c[0] for c in R.SPECTRAL_CONFIGS)


@pytest.mark.parametrize("config", R.SPECTRAL_CONFIGS)
def test_spectral_fp32_within_half(config):
    basis, melw = R.spectral_tables(config)
    n_fft, hop, n_mels = config
    for case in [c for c in R.spectral_cases() if c[0] == config]:
        cfg = R.spectral_cfg(*case[:5])
        B = case[5]
        for n in R.spectral_lengths(n_fft, hop, cfg["pad_mode"]):
            x = R.spectral_input(case, n)
            assert x.shape == (B, n) and (B == 1 or not np.array_equal(x[0], x[1]))
            ref, mel = R.spectral_ref(x, cfg, basis, melw)
            got, _ = R.spectral_ref(x, cfg, basis, melw, F32)
            T = 1 + n // hop
            assert ref.shape == ((B, T, n_mels) if cfg["out_layout"] == "btm" else (B, n_mels, T))
            # no element between 0 and the floor's edge: the exact floor comparison applies to silence alone
            assert bool((mel > 1.001 * cfg["amin"]).all()), (case, n, float(mel.min()))
            gate = R.spectral_gate(mel, cfg)
            assert bool((np.abs(got - ref) <= gate / 2).all()), (case, n, float((np.abs(got - ref) / gate).max()))
            if cfg["log_kind"] == "transforms_16000" and n >= n_fft:          # the image is not all clipped
                assert bool(((ref > 0) & (ref < 1)).any())


@pytest.mark.parametrize("log_kind", ("db", "transforms_16000"))
def test_the_silent_row_is_at_the_floor(log_kind):
    cfg, x = R.silent_case(log_kind)
    basis, melw = R.spectral_tables(R.SILENT_CONFIG)
    ref, mel = R.spectral_ref(x, cfg, basis, melw)
    assert not x[1].any() and bool((mel[1] == 0).all()) and bool((mel[0] > 1.001 * cfg["amin"]).all()) and bool((mel[2] > 1.001 * cfg["amin"]).all())
    assert bool((ref[1] == R.spectral_floor(cfg)).all()) or log_kind == "db" and float(np.abs(ref[1] - R.spectral_floor(cfg)).max()) < 1e-6
    assert (x.shape[1] + cfg["n_fft"]) % 4 != 0          # the padded rows' pitch is not their length
    got, _ = R.spectral_ref(x, cfg, basis, melw, F32)
    assert bool((np.abs(got - ref) <= R.spectral_gate(mel, cfg) / 2).all())
    assert R.check_floor(got, mel, cfg) == got[1].size and R.check_floor(ref, mel, cfg) == got[1].size


def test_the_loud_row_clips_to_one():
    cfg, x = R.loud_case()
    basis, melw = R.spectral_tables(R.SILENT_CONFIG)
    assert 2e4 < float(np.abs(x).max()) < 32768
    _, mel = R.spectral_ref(x, cfg, basis, melw)
    pre = R.logmel_ref(mel.reshape(-1, cfg["n_mels"]), 1, mel.shape[1], cfg["n_mels"], 1, cfg["amin"], 0.0, 0, clip=False)
    assert float(pre.min()) >= 1.001
    got, _ = R.spectral_ref(x, cfg, basis, melw, F32)
    assert bool((got == 1).all())
