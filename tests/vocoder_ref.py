"""Float64 references, inputs and shape lists of the 1-D vocoder operator tests (tests/test_gpu_vocoder_ops.py; checked on the
CPU by tests/test_vocoder_ref.py).  Plain torch on the CPU, nothing from the library."""
import functools
import math

import torch
import torch.nn.functional as F

TOL = {"f32": 2e-5, "bf16x3": 2e-4}          # the project's operator tolerances (rel-max)
SNAKE_TOL = 1e-5

# ---- shapes shared by the GPU tests and the CPU checks ----------------------------------------------------------------
B = 3
SNAKE_TILED_C = (32, 64, 128, 192)           # snake_aa_tiled_kernel<32> (C == 32) and <64> (C % 64 == 0)
SNAKE_UNTILED_C = (48, 96)                   # snake_aa_kernel
SNAKE_L = (1, 2, 5, 6, 7, 63, 64, 65, 127, 128, 129, 333)
SNAKE_BITWISE = ((64, 48), (32, 24))         # (tiled C, untiled C cut from its first channels)
SNAKE_BITWISE_L = (1, 65, 333)

MRF_C = (32, 64, 48)                         # 32 / 64: halo kernels in bf16x3; 48: never
MRF_PAIRS = ((3, 1, 3, 1), (3, 5, 3, 1), (7, 3, 7, 1), (11, 5, 11, 1), (3, 1, 11, 1))       # (k1, d1, k2, d2)
MRF_SINGLES = ((3, 1), (5, 6), (7, 12))      # (k, d) of a ResBlock2 step, C = 64; (7, 12) is past the halo limit
MRF_EPILOGUES = ((1.0, False), (1.0 / 3.0, False), (1.0, True), (1.0 / 3.0, True))          # (out_scale, accumulate)
HALO_HMAX, HALO_HMAX2 = 32, 16               # halo_conv1d.hip: d (k - 1) / 2 <= HMAX; the pair's d2 (k2 - 1) <= HMAX2

CONVTR = ((64, 32, 8, 8, 17), (64, 32, 24, 8, 17), (32, 16, 6, 2, 5), (64, 32, 16, 8, 1), (64, 32, 4, 2, 2), (96, 1, 8, 4, 33),
          (33, 7, 4, 2, 10), (128, 64, 3, 1, 9))                                              # (Cin, Cout, k, s, L)
CONVTR_REFUSED = ((7, 2, "multiple of the stride"), (4, 1, "must be even"), (32, 8, "carry"), (10, 2, "carry"))   # (k, s, rule)


def tile_out(C, k2=1, d2=1):
    """Output rows of one tile of the halo kernels: TLo = TL - d2 (k2 - 1), TL = 256 at C = 32, else 128."""
    return (256 if C == 32 else 128) - d2 * (k2 - 1)


def mrf_lengths(C, k2=1, d2=1):
    t = tile_out(C, k2, d2)
    return (1, 2, t - 1, t, t + 1, 2 * t + 1)


def halo_pair_covers(C, k1, d1, k2, d2):
    return C in (32, 64) and d1 * (k1 - 1) // 2 <= HALO_HMAX and d2 * (k2 - 1) <= HALO_HMAX2


def halo_single_covers(C, k, d):
    return C in (32, 64) and d * (k - 1) // 2 <= HALO_HMAX


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_max(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---- anti-aliased snake ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kaiser_sinc12():
    """12-tap Kaiser-windowed sinc, cutoff 0.25, half width 0.3, from the formula in double; rounded to fp32 as the library
    keeps them.  -> float64 tensor [12]."""
    cutoff, half_width, ks = 0.25, 0.3, 12
    A = 2.285 * (ks // 2 - 1) * math.pi * 4 * half_width + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    n = torch.arange(ks, dtype=torch.float64)
    r = 2.0 * n / (ks - 1) - 1.0
    window = torch.special.i0(beta * torch.sqrt(1.0 - r * r)) / torch.special.i0(torch.tensor(beta, dtype=torch.float64))
    t = n - ks // 2 + 0.5
    f = 2 * cutoff * window * torch.sinc(2 * cutoff * t)
    return (f / f.sum()).float().double()


def snake_aa_ref(x, alpha, beta, logscale):
    """Activation1d: replicate-pad 5, 2x up (transposed FIR, gain 2, crop 15), x + sin^2(alpha x) / (beta + 1e-9),
    replicate-pad (5, 6), FIR with stride 2.  x [B, C, L]; float64 throughout."""
    f = kaiser_sinc12()
    x = x.double()
    Bn, C, L = x.shape
    a, b = alpha.double()[None, :, None], beta.double()[None, :, None]
    if logscale:
        a, b = torch.exp(a), torch.exp(b)
    idx = (torch.arange(L + 10) - 5).clamp(0, L - 1)
    xp = x[:, :, idx]                                              # [B, C, L + 10]
    full = torch.zeros(Bn, C, 2 * (L + 10) + 10, dtype=torch.float64)
    for k in range(12):                                            # full[2 i + k] += f[k] xp[i]
        full[:, :, k:k + 2 * (L + 10):2] += f[k] * xp
    up = 2.0 * full[:, :, 15:15 + 2 * L]
    z = up + torch.sin(a * up) ** 2 / (b + 1e-9)
    idx = (torch.arange(2 * L + 11) - 5).clamp(0, 2 * L - 1)
    zp = z[:, :, idx]
    out = torch.zeros(Bn, C, L, dtype=torch.float64)
    for j in range(12):                                            # out[l] = sum_j f[j] zp[2 l + j]
        out += f[j] * zp[:, :, j:j + 2 * L:2]
    return out


def snake_params(C, seed=0):
    return torch.randn(C, generator=gen(380 + seed)) * 0.3, torch.randn(C, generator=gen(390 + seed)) * 0.3


def snake_input(C, L, kind):
    """`randn`, or `spike`: a ramp plus 50 at positions 0, L - 1, 63, 64 -- a wrong clamp or a row of the neighbouring tile then
    moves the answer by far more than the tolerance."""
    if kind == "randn":
        return torch.randn(B, C, L, generator=gen(37 + 7 * C + L))
    x = torch.arange(L, dtype=torch.float32)[None, None, :] * 0.01 + torch.arange(C, dtype=torch.float32)[None, :, None] * 0.003
    x = x + torch.arange(B, dtype=torch.float32)[:, None, None] * 0.1
    for p in (0, L - 1, 63, 64):
        if 0 <= p < L:
            x[:, :, p] += 50.0
    return x.contiguous()


@functools.lru_cache(maxsize=64)
def snake_case(C, L, kind, logscale):
    x = snake_input(C, L, kind)
    al, be = snake_params(C)
    return x, al, be, snake_aa_ref(x, al, be, logscale)


def snake_large_case(C, L=333):
    """alpha * up up to about 200: x ~ 20 randn, alpha = 10, no logscale."""
    x = 20.0 * torch.randn(B, C, L, generator=gen(41 + C))
    al = torch.full((C,), 10.0)
    be = 0.5 + torch.rand(C, generator=gen(42 + C))
    return x, al, be


def snake_fp32_restatement(x, al, be, logscale):
    """The oracle's chain in float32 on the CPU: the baseline the device's large-argument bound is measured from."""
    from oracle import vocoder as O
    filt = O.kaiser_sinc_filter1d(0.25, 0.3, 12)
    return O.downsample1d(O.snake(O.upsample1d(x.float(), filt), al.float(), be.float(), logscale), filt)


# ---- MRF pair / single conv --------------------------------------------------------------------------------------------
def _leaky(x, s):
    return x if s == 0 else F.leaky_relu(x, s)


def _same_conv(x, w, b, k, d):
    return F.conv1d(x, w, b, padding=d * (k - 1) // 2, dilation=d)


def mrf_pair_ref(x, w1, b1, k1, d1, s1, w2, b2, k2, d2, s2, out_scale, out_prev):
    """out_prev + out_scale * (c2(leaky(c1(leaky(x, s1)), s2)) + x); w2 None: out_prev + out_scale * (c1(leaky(x, s1)) + x);
    out_prev None: no accumulate.  "same" zero padding; float64."""
    x = x.double()
    t = _same_conv(_leaky(x, s1), w1.double(), None if b1 is None else b1.double(), k1, d1)
    if w2 is not None:
        t = _same_conv(_leaky(t, s2), w2.double(), None if b2 is None else b2.double(), k2, d2)
    y = out_scale * (t + x)
    return y if out_prev is None else out_prev.double() + y


def split_bf16(x):
    """fp32 -> (hi, lo) as float64: hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


def _conv_bf16x3(conv, a, w):
    """hi*hi + hi*lo + lo*hi of the split operands, accumulated in float64; conv(a, w) is linear in both."""
    ah, al = split_bf16(a)
    wh, wl = split_bf16(w)
    return conv(ah, wh) + conv(ah, wl) + conv(al, wh)


def mrf_pair_emulated(x, w1, b1, k1, d1, s1, w2, b2, k2, d2, s2, out_scale, out_prev):
    """mrf_pair_ref with the bf16x3 engines' operand rounding (the intermediate is fp32, then split again)."""
    t = _conv_bf16x3(lambda a, w: _same_conv(a, w, None, k1, d1), _leaky(x.float(), s1), w1)
    if b1 is not None:
        t = t + b1.double()[None, :, None]
    if w2 is not None:
        t = _conv_bf16x3(lambda a, w: _same_conv(a, w, None, k2, d2), _leaky(t.float(), s2), w2)
        if b2 is not None:
            t = t + b2.double()[None, :, None]
    y = out_scale * (t + x.double())
    return y if out_prev is None else out_prev.double() + y


def mrf_inputs(C, k1, d1, k2, d2, L, kind="randn"):
    """x, w1, b1, w2, b2, out_prev (k2 = 0: no second conv).  kinds: `randn`; `bias3`: b1 = 3.0 -- an intermediate that were
    c1(0) + b1 instead of zero outside [0, L) would move the first and last (k2 - 1) / 2 outputs of every sample by O(1);
    `spike`: x is zero except 100 at the last position of sample 0 and the first of sample 1."""
    seed = 1000 * C + 100 * k1 + 10 * d1 + k2 + 7 * L
    if kind == "spike":
        x = torch.zeros(B, C, L)
        x[0, :, L - 1] = 100.0
        x[1, :, 0] = 100.0
    else:
        x = torch.randn(B, C, L, generator=gen(seed))
    w1 = torch.randn(C, C, k1, generator=gen(seed + 1)) / math.sqrt(C * k1)
    b1 = torch.full((C,), 3.0) if kind == "bias3" else torch.randn(C, generator=gen(seed + 2))
    w2 = b2 = None
    if k2:
        w2 = torch.randn(C, C, k2, generator=gen(seed + 3)) / math.sqrt(C * k2)
        b2 = torch.randn(C, generator=gen(seed + 4))
    out_prev = torch.randn(B, C, L, generator=gen(seed + 5))
    return x, w1, b1, w2, b2, out_prev


SLOPE = 0.1


@functools.lru_cache(maxsize=64)
def mrf_case(C, k1, d1, k2, d2, L, kind, out_scale, accumulate):
    """(inputs, float64 reference) of one operator case, shared by the precision modes."""
    x, w1, b1, w2, b2, prev = mrf_inputs(C, k1, d1, k2, d2, L, kind)
    ref = mrf_pair_ref(x, w1, b1, k1, d1, SLOPE, w2, b2, k2, d2, SLOPE, out_scale, prev if accumulate else None)
    return (x, w1, b1, w2, b2, prev), ref


# ---- transposed conv ---------------------------------------------------------------------------------------------------
def conv_transpose1d_ref(x, w, b, s, leaky):
    k = w.shape[2]
    return F.conv_transpose1d(_leaky(x.double(), leaky), w.double(), b.double(), stride=s, padding=(k - s) // 2)


def convtr_emulated(x, w, b, s, leaky):
    k = w.shape[2]
    y = _conv_bf16x3(lambda a, ww: F.conv_transpose1d(a, ww, None, stride=s, padding=(k - s) // 2), _leaky(x.float(), leaky), w)
    return y + b.double()[None, :, None]


def convtr_inputs(Cin, Cout, k, s, L):
    seed = 25 + Cin + 3 * k + L
    x = torch.randn(B, Cin, L, generator=gen(seed))
    w = torch.randn(Cin, Cout, k, generator=gen(seed + 1)) / math.sqrt(Cin * k / s)
    b = torch.randn(Cout, generator=gen(seed + 2))
    return x, w, b


def convtr_impulse(Cin, Cout, k, s, L):
    """x = one 1 at (b = 1, ci = 3, l = L - 1): the output is bias everywhere, plus w[3, :, t] at position (L - 1) s - pad + t."""
    _, w, b = convtr_inputs(Cin, Cout, k, s, L)
    x = torch.zeros(B, Cin, L)
    x[1, 3, L - 1] = 1.0
    out = b.double()[None, :, None].repeat(B, 1, L * s)
    pad = (k - s) // 2
    for t in range(k):
        j = (L - 1) * s - pad + t
        if 0 <= j < L * s:
            out[1, :, j] += w[3, :, t].double()
    return x, w, b, out
