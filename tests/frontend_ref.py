"""References and inputs of the waveform front-end operator tests (tests/test_gpu_frontend_ops.py on the device,
tests/test_frontend_ref.py on the CPU): the small kernels of csrc/spectral.hip, the Spectral and Resampler handles and
DeviceMelTransform.resample, each restated in float64 with plain numpy from the formulas in the kernels' comments, and the seeded
inputs and shape lists both test files use.  Nothing here touches the library's device path; the host-side tables the front ends
are built from (mel.dft_basis, mel.mel_filterbank, the two resampler banks) are inputs of the references, as they are of the
handles."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64

# ---------------------------------------------------------------------------------------------------- gates
TOL_POWER = 1e-6          # relative, per element: three roundings, one contracted fma at most, sqrtf within 1 ulp: < 4 ulp = 4.8e-7
FLT_MIN = float(np.finfo(np.float32).tiny)
TOL_DB = 1e-4             # absolute dB: log10f within 2 ulp at |log10| <= 14, times 10, plus the product's rounding at 140: 3.4e-5
TOL_T16K = 1e-6           # absolute, the [0, 1] mel image
TOL_AFFINE = 1e-6         # of max|ref|
TOL_REDUCE = 2e-5         # of max|ref|: the project's gate for a reduction
TOL_RESAMPLE = 1e-5       # rel-max: the project's resampler gate
TOL_PLACE = 1e-6          # absolute: one output of a unit impulse is one float32 bank entry

# ---------------------------------------------------------------------------------------------------- shapes
PAD_B = (1, 3)
PAD_CASES = ((5, 4, 4), (33, 32, 32), (37, 7, 7 + 3), (200, 0, 16), (1, 6, 9))          # (n, left, right); (1, 6, 9): zeros only
PAD_REFUSED = ((4, 4, 2), (4, 2, 4))                                                     # reflect with n == left, n == right
POWER_ROWS = (1, 5, 300)
POWER_NF = (33, 65, 513)
LOGMEL_B = (1, 2)
LOGMEL_FRAMES = (1, 7)
LOGMEL_MELS = (8, 13, 80)
LOGMEL_PAD_VALUE = 3e4                                                                   # what the 3 spare floats of a mel row hold
LOGMEL_KINDS = ((0, 1e-10), (1, 1e-5))                                                   # (log_kind, amin); ref = 1
AFFINE_SHAPES = ((3, 64), (19, 13), (257, 64))                                           # (B * T, F)
POOL_SHAPES = ((1, 1, 1, 4), (3, 2, 2, 100), (2, 31, 4, 300), (1, 7, 1, 260))            # (B, T, F, C)
SIM_NA, SIM_NT, SIM_D, SIM_SCALE = (1, 3), (1, 5), (1, 63, 64, 65, 1024), (1.0, 1.0 / 0.07)

SPECTRAL_CONFIGS = ((64, 16, 8), (128, 32, 16), (256, 64, 20), (64, 4, 8), (64, 64, 8), (64, 128, 8))      # (n_fft, hop, n_mels)
SPECTRAL_SR, SPECTRAL_FMIN, SPECTRAL_FMAX = 16000, 125.0, 7600.0
SPECTRAL_AMIN = {"db": 1e-10, "transforms_16000": 1e-5}


def spectral_cases():
    """(config, pad_mode, power, log_kind, out_layout, B): four per configuration, 24 in all, in which every value of every
    setting meets every n_fft, and both powers meet both layouts."""
    out = []
    for i, c in enumerate(SPECTRAL_CONFIGS):
        a, b = ("bmt", "btm") if i % 2 == 0 else ("btm", "bmt")
        out += [(c, "reflect", 2, "db", a, 1), (c, "constant", 1, "transforms_16000", b, 3),
                (c, "reflect", 1, "db", b, 3), (c, "constant", 2, "transforms_16000", a, 1)]
    return out


def spectral_lengths(n_fft, hop, pad_mode):
    """n_fft / 2 + 1 (the shortest reflect pad), 3 hop + 5, 1000, and -- where the padding takes them -- one frame (hop - 1), one
    sample, and hop."""
    ns = sorted({n_fft // 2 + 1, 3 * hop + 5, 1000, hop - 1, 1, hop})
    return [n for n in ns if pad_mode == "constant" or n > n_fft // 2]


def spectral_cfg(config, pad_mode, power, log_kind, out_layout):
    n_fft, hop, n_mels = config
    return dict(n_fft=n_fft, hop=hop, n_mels=n_mels, pad_mode=pad_mode, power=power, log_kind=log_kind,
                amin=SPECTRAL_AMIN[log_kind], ref=1.0, out_layout=out_layout)


@functools.lru_cache(maxsize=None)
def spectral_tables(config):
    from audiogpt_amd import mel
    n_fft, hop, n_mels = config
    return mel.dft_basis(n_fft), mel.mel_filterbank(sr=SPECTRAL_SR, n_fft=n_fft, n_mels=n_mels, fmin=SPECTRAL_FMIN, fmax=SPECTRAL_FMAX)


RESAMPLE_RATIOS = ((16000, 44100), (44100, 16000), (48000, 16000), (22050, 44100), (16000, 48000), (48000, 44100))
RESAMPLE_REDUCED = ((160, 441), (441, 160), (3, 1), (1, 2), (1, 3), (160, 147))
RESAMPLE_BANKS = ((441, 174), (160, 475), (1, 41), (2, 15), (3, 15), (147, 174))
RESAMPLE_B = (1, 3)


def resample_lengths(orig):
    return sorted({1, max(orig - 1, 2), orig, orig + 1, 2 * orig + 3, 1500})


@functools.lru_cache(maxsize=None)
def sinc_bank(orig_freq, new_freq):
    from audiogpt_amd import clap
    return clap.sinc_resample_kernel(orig_freq, new_freq)


DMT_SR = (44100, 22050, 48000, 24000, 8000)
DMT_TARGET = 16000
DMT_CARRY_SR = (44100, 22050)


def dmt_lengths(sr):
    return (3000, 3 * (sr // math.gcd(sr, DMT_TARGET)), 1)


# ---------------------------------------------------------------------------------------------------- inputs
TONES = (0.031, 0.127, 0.283)            # cycles per sample, one per batch row
NOISE = (0.02, 0.1, 0.3)                 # noise level, one per batch row


def wave(B, n, seed, level=1.0):
    """float32 [B, n]: row b is a tone of its own frequency plus noise of its own level."""
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=F64)
    rows = [0.5 * np.sin(2 * np.pi * TONES[b % 3] * t + 0.3 * b + 0.2) + NOISE[b % 3] * rng.randn(n) for b in range(B)]
    return (level * np.stack(rows)).astype(F32)


def spectral_input(case, n):
    """The waveform [B, n] of one of spectral_cases() at length n; the "transforms_16000" cases are 30 times louder, which puts
    their mel image inside (0, 1) instead of at its lower clip."""
    (n_fft, hop, n_mels), pad_mode, power, log_kind, layout, B = case
    return wave(B, n, 31 * n_fft + 7 * hop + n + power, level=30.0 if log_kind == "transforms_16000" else 1.0)


SILENT_CONFIG = SPECTRAL_CONFIGS[1]
SILENT_N = 1001          # n + n_fft is odd: the padded rows' pitch (rounded up to 4) is not their length


def silent_case(log_kind):
    """(cfg, x [3, n]) with row 1 silent."""
    cfg = spectral_cfg(SILENT_CONFIG, "reflect", 2 if log_kind == "db" else 1, log_kind, "bmt" if log_kind == "db" else "btm")
    x = wave(3, SILENT_N, 77, level=30.0 if log_kind == "transforms_16000" else 1.0)
    x[1] = 0
    return cfg, x


def loud_case():
    """(cfg, x [1, n]) at int16 scale under "transforms_16000": every element of the image clips to 1."""
    cfg = spectral_cfg(SILENT_CONFIG, "reflect", 1, "transforms_16000", "bmt")
    return cfg, wave(3, SILENT_N, 78, level=2e4)[2:3].copy()


def power_input(rows, nf, ldy, seed):
    """float32 [rows, ldy]: magnitudes log-uniform over 1e-6 .. 1e15 with random signs; planted in row 0: re = im = 0 (column 0), a
    denormal pair (column 1), a denormal beside 1 (column 2), the largest magnitude (column 3)."""
    rng = np.random.RandomState(seed)
    y = (10.0 ** rng.uniform(-6, 15, (rows, ldy)) * rng.choice([-1.0, 1.0], (rows, ldy))).astype(F32)
    for col, (re, im) in enumerate(((0.0, 0.0), (1e-40, -3e-41), (1e-40, 1.0), (1e15, -1e15))):
        y[0, col], y[0, nf + col] = re, im
    return y


def logmel_input(B, frames, n_mels, ldmel, kind, amin, seed):
    """float32 [B * frames, ldmel]: log-uniform over 1e-14 .. 1e4, the spare columns LOGMEL_PAD_VALUE; planted at the start of row
    0: amin, the float below it, half of it, 0; for kind 1 also values that land below 0 (3e-5) and above 1 (20, 5e3) before the
    clip."""
    rng = np.random.RandomState(seed)
    x = (10.0 ** rng.uniform(-14, 4, (B * frames, ldmel))).astype(F32)
    a = F32(amin)
    plant = [a, np.nextafter(a, F32(0)), a / F32(2), F32(0)] + ([F32(3e-5), F32(20.0), F32(5e3)] if kind == 1 else [])
    x.reshape(-1)[:len(plant)] = plant          # (n_mels >= 8 > len(plant): all inside row 0's bins)
    x[:, n_mels:] = LOGMEL_PAD_VALUE
    return x


def affine_input(rows, F, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(rows * F) * 30.0 - 40.0).astype(F32)          # log-mel-like dB values
    return x, rng.uniform(0.05, 2.0, F).astype(F32), (rng.randn(F) * 3.0).astype(F32)


def pool_input(B, T, F, C, seed):
    """float32 [B, T, F, C] channels-last: non-negative noise (as after a ReLU); channel 1 negative everywhere, channel 2 constant,
    channel 3 an offset of 1e3 plus unit noise."""
    rng = np.random.RandomState(seed)
    x = np.abs(rng.randn(B, T, F, C))
    x[..., 1] = -0.25 - np.abs(rng.randn(B, T, F))
    x[..., 2] = 0.7
    x[..., 3] = 1e3 + rng.randn(B, T, F)
    return x.astype(F32)


def similarity_input(Na, Nt, D, seed):
    """Rows of different norms; where D >= 2, audio row 0 and text row 0 are orthogonal."""
    rng = np.random.RandomState(seed)
    a = (rng.randn(Na, D) * (1.0 + 2.0 * np.arange(Na))[:, None]).astype(F32)
    t = (rng.randn(Nt, D) * (0.5 + np.arange(Nt))[:, None]).astype(F32)
    if D >= 2:
        a[0], t[0] = 0, 0
        a[0, 0::2] = 1.5
        t[0, 1::2] = -2.0
    return a, t


# ---------------------------------------------------------------------------------------------------- references
def pad_ref(x, left, right, mode, ldo):
    """x [B, n] -> float32 [B, ldo]: np.pad by (left, right), the columns behind it zero.  mode: "constant" | "reflect"."""
    x = np.asarray(x, F32)
    p = np.pad(x, ((0, 0), (left, right)), mode=mode)
    out = np.zeros((x.shape[0], ldo), F32)
    out[:, :p.shape[1]] = p
    return out


def power_ref(y, nf, ldm, power2, dtype=F64):
    y = np.asarray(y).astype(dtype)
    re, im = y[:, :nf], y[:, nf:2 * nf]
    v = re * re + im * im
    out = np.zeros((y.shape[0], ldm), dtype)
    out[:, :nf] = v if power2 else np.sqrt(v)
    return out


def power_floor(power2):
    """What float32 cannot resolve: where re^2 + im^2 is below the smallest normal float32 the sum has lost its relative precision
    (or is flushed to zero), an absolute FLT_MIN of the power and sqrt(FLT_MIN) of the magnitude."""
    return FLT_MIN if power2 else math.sqrt(FLT_MIN)


def logmel_ref(mel, B, frames, n_mels, kind, amin, ref_db, layout, dtype=F64, clip=True):
    """mel [B * frames, ldmel] -> [B, frames, n_mels] (layout 0) or [B, n_mels, frames] (layout 1); amin and ref_db as the float32
    values the kernel receives.  clip=False: kind 1 before its clip to [0, 1]."""
    v = np.maximum(np.asarray(mel)[:, :n_mels].astype(dtype), dtype(F32(amin)))
    if kind == 0:
        o = dtype(10) * np.log10(v) - dtype(F32(ref_db))
    else:
        o = (np.log10(v) * dtype(20) - dtype(20) + dtype(100)) / dtype(100)
        if clip:
            o = np.clip(o, 0, 1)
    o = o.reshape(B, frames, n_mels)
    return o if layout == 0 else np.ascontiguousarray(o.transpose(0, 2, 1))


def affine_ref(x, F, scale, shift, dtype=F64):
    x = np.asarray(x).astype(dtype).reshape(-1, F)
    return (x * np.asarray(scale).astype(dtype) + np.asarray(shift).astype(dtype)).reshape(-1)


def pool_ref(x, dtype=F64):
    """x [B, T, F, C] -> [B, C]: max_t mean_f + mean_t mean_f."""
    m = np.asarray(x).astype(dtype).mean(axis=2)
    return m.max(axis=1) + m.mean(axis=1)


def similarity_ref(a, t, scale, dtype=F64):
    return dtype(scale) * (np.asarray(a).astype(dtype) @ np.asarray(t).astype(dtype).T)


def frames_of(xp, n_frames, length, pitch):
    """xp [B, total] -> [B, n_frames, length]: frame t is xp[:, t pitch : t pitch + length]."""
    idx = pitch * np.arange(n_frames)[:, None] + np.arange(length)[None, :]
    return xp[:, idx]


def spectral_ref(x, cfg, basis, melw, dtype=F64):
    """Spectral.forward: x [B, n] -> (log-mel in cfg's layout, linear mel [B, frames, n_mels]).  Centre padding by n_fft / 2,
    frames xp[t hop : t hop + n_fft] for t < 1 + n // hop, the framed DFT as a product with the given float32 basis (window folded
    in), power, the mel product, the logarithm."""
    x = np.asarray(x, F32)
    B, n = x.shape
    n_fft, hop, nf, n_mels = cfg["n_fft"], cfg["hop"], cfg["n_fft"] // 2 + 1, cfg["n_mels"]
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode=cfg["pad_mode"]).astype(dtype)
    T = 1 + n // hop
    y = frames_of(xp, T, n_fft, hop) @ np.asarray(basis).astype(dtype).T                    # [B, T, 2 nf]
    mag = power_ref(y.reshape(B * T, 2 * nf), nf, nf, cfg["power"] == 2, dtype)
    mel = (mag @ np.asarray(melw).astype(dtype).T).reshape(B, T, n_mels)
    kind = {"db": 0, "transforms_16000": 1}[cfg["log_kind"]]
    amin = F32(cfg["amin"])
    ref_db = F32(10) * np.log10(np.maximum(amin, F32(cfg.get("ref", 1.0))))
    out = logmel_ref(mel.reshape(B * T, n_mels), B, T, n_mels, kind, amin, ref_db, 0 if cfg["out_layout"] == "btm" else 1, dtype)
    return out, mel


def spectral_floor(cfg):
    """The value of an element whose linear mel is at or below amin."""
    if cfg["log_kind"] == "db":
        return 10.0 * math.log10(float(F32(cfg["amin"]))) - 10.0 * math.log10(max(float(F32(cfg["amin"])), cfg.get("ref", 1.0)))
    return 0.0


def spectral_gate(mel, cfg):
    """Per-element bound on |device - spectral_ref| in cfg's layout: the 2e-5 reduction gate on the linear mel, relative to the
    largest mel of the frame, carried through 10 log10 (d dB = 4.343 dm / m) or 20 log10 / 100 (0.0869 dm / m), plus the logarithm
    kernel's own gate.  Elements at the floor (mel <= amin) get the logarithm's gate alone, and `check_floor` on top."""
    db = cfg["log_kind"] == "db"
    m_max = mel.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (4.343 if db else 0.0869) * TOL_REDUCE * m_max / mel
    g = np.where(mel <= float(F32(cfg["amin"])), 0.0, g) + (TOL_DB if db else TOL_T16K)
    return g if cfg["out_layout"] == "btm" else np.ascontiguousarray(g.transpose(0, 2, 1))


def check_floor(got, mel, cfg):
    """Every element of `got` (cfg's layout) whose reference linear mel is at or below amin holds the floor: 0.0 exactly for
    "transforms_16000", one bit-identical value within TOL_DB of 10 log10(amin) - ref_db for "db".  -> how many there are."""
    at = mel <= float(F32(cfg["amin"]))
    at = at if cfg["out_layout"] == "btm" else at.transpose(0, 2, 1)
    v = np.asarray(got)[at]
    if v.size:
        assert bool((v == v[0]).all()), "the floor is not one value"
        assert float(v[0]) == 0.0 if cfg["log_kind"] != "db" else abs(float(v[0]) - spectral_floor(cfg)) <= TOL_DB, float(v[0])
    return int(v.size)


def resample_ref(x, bank, width, orig, new, dtype=F64):
    """Resampler.forward: x [B, n] -> [B, ceil(new n / orig)]: zero padding by (width, width + orig), n // orig + 1 frames of
    2 width + orig samples at stride orig, each times bank^T, flattened in (frame, phase) order."""
    x = np.asarray(x, F32)
    B, n = x.shape
    xp = np.pad(x, ((0, 0), (width, width + orig))).astype(dtype)
    y = frames_of(xp, n // orig + 1, 2 * width + orig, orig) @ np.asarray(bank).astype(dtype).T
    return y.reshape(B, -1)[:, :-(-new * n // orig)]


def resampy_ref(x, sr, dtype=F64):
    """mel.librosa_resample to DMT_TARGET as resample_ref states it: the periodic resampy bank, the carry outputs from the
    one-phase carry kernel, and zeros from int(n ratio) on.  x [n] -> [ceil(n ratio)]."""
    from audiogpt_amd import mel
    g = math.gcd(sr, DMT_TARGET)
    orig, new = sr // g, DMT_TARGET // g
    bank, width = mel.resampy_kernel_bank(sr, DMT_TARGET)
    n = x.shape[0]
    ratio = float(DMT_TARGET) / float(sr)
    n_resampy, n_fixed = int(n * ratio), int(np.ceil(n * ratio))
    y = resample_ref(x[None], bank, width, orig, new, dtype)[0][:n_fixed].copy()
    t = mel.resampy_carries(n_resampy, sr, DMT_TARGET)
    if t.size:
        y[t] = resample_ref(x[None], mel.resampy_carry_kernel(sr, DMT_TARGET), width, orig, 1, dtype)[0][t // new]
    y[n_resampy:] = 0
    return y


@functools.lru_cache(maxsize=None)
def dmt_case(sr, n):
    """(x float32 [n], oracle.resampy.librosa_resample(x in float64, sr, DMT_TARGET)): the scalar time-register loop, computed once."""
    from oracle import resampy as O
    x = wave(1, n, 1000 + sr // 50 + n)[0]
    return x, np.asarray(O.librosa_resample(x.astype(F64), sr, DMT_TARGET), F64)


def rel_max(got, ref):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))
