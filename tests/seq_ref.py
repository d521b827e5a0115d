"""Host-side yardstick for the row operators of DiffSinger's sequence models (csrc/pitch.hip, fs2.hip, row_device.h through
maa_op_seq_rows, and the long-sequence tests through the model handles): float64 references written from the formulas in the
kernels' comments, and the seeded input builders that tests/test_gpu_seq_ops.py and tests/test_seq_ref.py share, so that the CPU
test and the GPU test see the same tensors.  Nothing here calls the library.

Every reference takes `dtype`: float64 is the yardstick, float32 is torch's own evaluation of the same formula, which
tests/test_seq_ref.py holds to half of the GPU tolerance."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import fs2_pitch_ref as FP
from tests import fs2_ref as FS
from tests import pe_ref as PE

TOL_ROW = 1e-5          # rel-max against float64: a LayerNorm or an elementwise affine
TOL_REDUCE = 2e-5       # ... followed by a reduction: the heads' dot products, the GroupNorm
EPS = 1e-5
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- frame mask

FM_BINS = (80, 256)
FM_ROWS = (1, 3, 5, 130)
FM_CONTENTS = ("zeros", "neg_zeros", "bin0", "bin_last", "last_lane", "denormal", "dense")
DENORMAL = 1.0e-45      # the smallest positive fp32


def frame_mask_input(M, rows, shift=0):
    """x [rows, M]: row r holds FM_CONTENTS[(r + shift) % 7].  last_lane: the one non-zero sits in the first bin of the last lane
    that holds any (lane M / 4 - 1: bin M - 4), so it is not the last bin."""
    x = torch.zeros(rows, M)
    dense = torch.randn(rows, M, generator=gen(300 + M + rows))
    for r in range(rows):
        kind = FM_CONTENTS[(r + shift) % len(FM_CONTENTS)]
        if kind == "neg_zeros":
            x[r] = -0.0
        elif kind == "bin0":
            x[r, 0] = -3.0
        elif kind == "bin_last":
            x[r, M - 1] = 2.0
        elif kind == "last_lane":
            x[r, M - 4] = 0.5
        elif kind == "denormal":
            x[r, M // 2 + 1] = DENORMAL
        elif kind == "dense":
            x[r] = dense[r]
    return x


def frame_mask_ref(x, dtype=F64):
    """mask [rows] = 0 where every bin is +-0, else 1 (pe.py:29-30: abs().sum(-1).eq(0)), as fp32 values."""
    return x.to(dtype).abs().sum(-1).ne(0).float()


def frame_mask_bits(x):
    """The same from the words: any bit but the sign set."""
    return (x.contiguous().view(torch.int32) & 0x7FFFFFFF).ne(0).any(-1).float()


# ---------------------------------------------------------------------------------------------------- masked affine

AM_C = (80, 256, 260, 1024)
AM_ROWS = (1, 5, 130)
HUGE = 1.0e30


def row_mask(rows, variant):
    """variant 0: zeros at row 0, the last row and rows r % 7 == 3; variant 1: all ones."""
    m = torch.ones(rows)
    if variant == 0:
        m[0] = m[rows - 1] = 0
        m[3::7] = 0
    return m


@functools.lru_cache(maxsize=None)
def affine_mask_input(C, rows, variant):
    """x [rows, C] ~ N(0, 1) with 1e30 planted on the masked rows, scale / shift [C], mask [rows]."""
    g = gen(400 + C + rows)
    x = torch.randn(rows, C, generator=g)
    scale, shift = 1.0 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    mask = row_mask(rows, variant)
    for r in torch.nonzero(mask == 0).flatten().tolist():
        x[r, (7 * r) % C] = HUGE
        x[r, C - 1] = -HUGE
    return x, scale, shift, mask


def affine_mask_ref(x, scale, shift, mask, dtype=F64):
    """out = (x * scale + shift) * mask[row]; scale None: x * mask[row]."""
    v = x.to(dtype)
    if scale is not None:
        v = v * scale.to(dtype) + shift.to(dtype)
    return v * mask.to(dtype)[:, None]


# ---------------------------------------------------------------------------------------------------- GroupNorm + ReLU + residual

GN_SHAPES = ((256, 16), (64, 16), (1024, 4))          # (C, groups): the model's, 4 channels per group, 256 per group
GN_T = (1, 3, 64, 257, 1100)
GN_B = 3
GN_SCALE, GN_OFFSET = (1.0, 10.0, 0.1), (0.5, -20.0, 3.0)      # per sample
GN_SIGMA = 1.7
GN_CASES = ("plain", "first_elem", "first_frame", "last_elem", "zero_sample")
GN_GROUP = 1            # the group the outliers go to


@functools.lru_cache(maxsize=None)
def gn_params(C):
    g = gen(500 + C)
    return torch.randn(C, generator=g), torch.randn(C, generator=g)


@functools.lru_cache(maxsize=None)
def gn_input(C, groups, T, case):
    """y, res [B, T, C]: y ~ N(0.3 + a per-channel offset, 1.7^2), then sample b times GN_SCALE[b] plus GN_OFFSET[b]; an outlier is
    1e3 times the sample's spread, planted in group 1 of every sample: its first element, its whole first frame, or its last
    element (the placements of tests/norm_ref.py); zero_sample: sample 1 is all zero."""
    g = gen(510 + C + T)
    y = torch.randn(GN_B, T, C, generator=g) * GN_SIGMA + 0.3 + 0.5 * torch.randn(C, generator=g)
    res = torch.randn(GN_B, T, C, generator=g)
    cpg = C // groups
    lo, hi = GN_GROUP * cpg, (GN_GROUP + 1) * cpg
    for b in range(GN_B):
        y[b] = y[b] * GN_SCALE[b] + GN_OFFSET[b]
        big = 1.0e3 * GN_SIGMA * GN_SCALE[b]
        if case == "first_elem":
            y[b, 0, lo] = big
        elif case == "first_frame":
            y[b, 0, lo:hi] = big
        elif case == "last_elem":
            y[b, T - 1, hi - 1] = -big
    if case == "zero_sample":
        y[1] = 0.0
    return y, res


def gn_compared(C, groups, T, case):
    """[C] bool: the channels a comparison of this case covers -- all of them, except that at T = 1 the first_frame placement
    fills the whole of group 1 with one value: its variance is 0, rstd = 1 / sqrt(eps) = 316 multiplies whatever rounding the mean
    of 1.7e3 .. 1.7e4 carries (one ulp is 1e-4 .. 1e-3), and torch's own fp32 GroupNorm is 4e-2 .. 7e-2 of max|ref| from float64
    there.  That group is left to the all-zero sample, whose constant group is exact; the other groups of the case are compared."""
    keep = torch.ones(C, dtype=torch.bool)
    if T == 1 and case == "first_frame":
        cpg = C // groups
        keep[GN_GROUP * cpg:(GN_GROUP + 1) * cpg] = False
    return keep


def gn_relu_res_ref(y, res, groups, gamma, beta, eps=EPS, dtype=F64):
    """out = res + relu(GroupNorm(y)), y / res channels-last [B, T, C], the statistics over all T frames of a sample."""
    n = F.group_norm(y.to(dtype).transpose(1, 2), groups, gamma.to(dtype), beta.to(dtype), eps).transpose(1, 2)
    return res.to(dtype) + F.relu(n)


# ---------------------------------------------------------------------------------------------------- positions + table gather

POS_C, POS_B = 256, 3
POS_T = (1, 63, 64, 65, 255, 256, 257, 511, 513, 1100)
POS_PATTERNS = {"a": ("none", "tail", "holes"), "b": ("all_zero", "last_only", "holes")}      # channel 0 of the three samples
POS_ALPHA = 0.7
POS_TABLE_ROWS = 2000
POS_GROW_ROWS, POS_GROW_T = 300, (299, 300, 513, 1100)


def channel0_live(T, pattern):
    """[T] bool: where channel 0 is non-zero."""
    live = torch.ones(T, dtype=torch.bool)
    if pattern == "tail":
        live[T - T // 3:] = False
    elif pattern == "holes":          # zero runs that straddle frames 63 / 64 and 255 / 256, and single zeros
        live[61:67] = False
        live[250:259] = False
        live[5::97] = False
    elif pattern == "all_zero":
        live[:] = False
    elif pattern == "last_only":
        live[:T - 1] = False
    else:
        assert pattern == "none"
    return live


@functools.lru_cache(maxsize=None)
def pos_input(T, key, C=POS_C):
    """x [B, T, C] dense ~ N(0, 1) with channel 0 zero by the sample's pattern (the all-zero sample: every channel)."""
    x = torch.randn(POS_B, T, C, generator=gen(600 + T))
    x[..., 0] = x[..., 0].abs() + 0.1
    for b, pattern in enumerate(POS_PATTERNS[key]):
        x[b, ~channel0_live(T, pattern), 0] = 0.0
        if pattern == "all_zero":
            x[b] = 0.0
    return x


def sinusoid_table_rounded(rows, dim):
    """pe_ref.sinusoid_table with every fp32 operation of get_embedding correctly rounded: the products in fp32 (exact to half an
    ulp by IEEE), exp / sin / cos in float64 and rounded once.  torch's own fp32 exp is good to 1 ulp and WHICH of the 128
    frequencies come out an ulp high depends on the build and on the thread count (measured: 3 on one host, 1, another one, on
    the next); one ulp in a frequency near 1 moves row p of the table by p * 1.2e-7, which is 1.2e-4 at p = 1056 -- seventeen
    times what the 1e-5 gate of pos_add leaves.  The table is a yardstick only when it does not depend on the host, so pos_add
    is held to this one; the library's host code (glibc's expf / sinf / cosf) is within one fp32 ulp of it on both hosts.
    tests/test_seq_ref.py holds torch's table to this one within what one ulp in a frequency allows."""
    half = dim // 2
    arg = torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1))
    freq = arg.double().exp().float()
    ang = torch.arange(rows, dtype=torch.float).unsqueeze(1) * freq.unsqueeze(0)
    tab = torch.cat([ang.double().sin(), ang.double().cos()], dim=1).float()
    tab[0] = 0
    return tab


def pos_add_ref(x, alpha, dtype=F64):
    """-> (pos [B, T] long, out = x + alpha * table[pos]) with the fp32 table of the reference, correctly rounded."""
    pos = PE.make_positions(x[..., 0])
    tab = sinusoid_table_rounded(x.shape[1] + 1, x.shape[2]).to(dtype)
    return pos, x.to(dtype) + torch.tensor(alpha, dtype=torch.float32).to(dtype) * tab[pos]


def make_positions_loop(ch0):
    out = torch.zeros(ch0.shape, dtype=torch.long)
    for b in range(ch0.shape[0]):
        n = 0
        for t in range(ch0.shape[1]):
            if float(ch0[b, t]) != 0.0:
                n += 1
                out[b, t] = n
    return out


# ---------------------------------------------------------------------------------------------------- predictor heads

HEAD_C = (4, 36, 256, 260, 384, 512, 516, 768, 1024)          # NR = 1: <= 256, 2: <= 512, 4: <= 1024, both edges of each
HEAD_ROWS = (1, 5, 130)
HEAD_CONST, HEAD_LARGE = 0.75, 50.0
F0_MEAN, F0_STD = 200.0, 50.0
DUR_CLEAR = 1e-4        # exp(xs) - 1 stays this fraction of exp(xs) away from a half-integer


def _head_draw(C, rows, n_out, seed):
    g = gen(seed)
    x = F.relu(torch.randn(rows, C, generator=g) + 0.3)          # non-negative, as after the convolution's ReLU
    if rows > 1:
        x[1] = HEAD_CONST                                        # var = 0: the output is beta . w + bias
    if rows > 2:
        x[2, (3 * C) // 4] = HEAD_LARGE                          # a single large channel
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = torch.randn(n_out, C, generator=g) / math.sqrt(C)
    if n_out == 2:
        bias = torch.tensor([7.5, 0.1])          # log2 f0 round 180 Hz, voicing logits of both signs
        w[0] *= 0.5
    else:
        bias = torch.tensor([1.5])               # durations 0 to about 30
        w *= 0.6
    return x, gamma, beta, w, bias, row_mask(rows, 0 if rows > 1 else 1)


def head_ref(x, gamma, beta, w, bias, dtype=F64):
    """LayerNorm over the row, then Linear(C, n_out) -> [rows, n_out]."""
    y = F.layer_norm(x.to(dtype), (x.shape[1],), gamma.to(dtype), beta.to(dtype), EPS)
    return F.linear(y, w.to(dtype), bias.to(dtype))


def logit_margin(pp):
    return TOL_REDUCE * float(pp.abs().max())


def pitch_head_clear(pp, mask):
    """No live voicing logit within the tolerance of 0."""
    return bool((pp[mask != 0, 1].abs() > logit_margin(pp)).all())


def dur_clear(xs):
    """Where exp(xs) - 1 is at least DUR_CLEAR * exp(xs) away from a half-integer."""
    e = xs.exp()
    frac = (e - 1.0) - torch.floor(e - 1.0)
    return (frac - 0.5).abs() >= DUR_CLEAR * e


def dur_head_clear(xs):
    return bool(dur_clear(xs).all())


@functools.lru_cache(maxsize=None)
def head_input(C, rows, n_out):
    """(x [rows, C], gamma, beta, w [n_out, C], bias, mask [rows]) from the first seed of 700 + C + rows, + 1000, ... whose float64
    reference is clear of the thresholds: no live voicing logit within the tolerance of 0 (n_out = 2), no exp(xs) - 1 within
    1e-4 exp(xs) of a half-integer (n_out = 1)."""
    for k in range(64):
        d = _head_draw(C, rows, n_out, 700 + C + rows + 1000 * k)
        ref = head_ref(*d[:5])
        if pitch_head_clear(ref, d[5]) if n_out == 2 else dur_head_clear(ref[:, 0] * d[5].double()):
            return d
    raise AssertionError("no seed clear of the thresholds")


def denorm_f0(pp, mask, pitch_norm, use_uv, dtype=F64):
    """denorm_f0 (pitch_utils.py:63-76) on pitch_pred [rows, 2]: pitch_norm 0: 2 ** v, 1: v * F0_STD + F0_MEAN."""
    v = pp[:, 0].to(dtype)
    f = 2.0 ** v if pitch_norm == 0 else v * F0_STD + F0_MEAN
    if use_uv:
        f = torch.where(pp[:, 1] > 0, torch.zeros_like(f), f)
    return torch.where(mask == 0, torch.zeros_like(f), f)


def out2dur(xs):
    """max(rint(exp(xs) - 1), 0) in float64 (torch.round is half to even)."""
    return torch.clamp(torch.round(xs.to(F64).exp() - 1.0), min=0).long()


# ---------------------------------------------------------------------------------------------------- long sequences

def length_regulate_loop(dur, T_mel):
    """mel2ph [B, T_mel]: frame p belongs to the first token whose running sum of max(dur, 0) exceeds p (1-based), else 0."""
    out = torch.zeros(dur.shape[0], T_mel, dtype=torch.long)
    for b in range(dur.shape[0]):
        p = 0
        for t in range(dur.shape[1]):
            for _ in range(max(int(dur[b, t]), 0)):
                if p < T_mel:
                    out[b, p] = t + 1
                p += 1
    return out


def length_regulate_ref(dur, T_mel):
    """fs2_ref.length_regulate on max(dur, 0), cut or zero-padded to T_mel frames."""
    m = FS.length_regulate(dur.long().clamp_min(0))
    if m.shape[1] >= T_mel:
        return m[:, :T_mel]
    return F.pad(m, [0, T_mel - m.shape[1]])


LR_T = (1, 255, 256, 257, 600)


@functools.lru_cache(maxsize=None)
def lr_dur():
    """dur [3, 600] int32, entries 0 .. 8: sample 0 zero from token 500 on, sample 1 with only its last token non-zero, sample 2
    with negative entries (which count as 0)."""
    d = torch.randint(0, 9, (3, 600), generator=gen(800), dtype=torch.int32)
    d[0, 500:] = 0
    d[1] = 0
    d[1, -1] = 7
    d[2, 11::13] = -3
    return d


def long_score(cfg, B, T, pad_from):
    """Seeded score inputs [B, T]; sample B - 1 is padding (token 0) from pad_from on."""
    g = gen(810 + T)
    tok = torch.randint(1, cfg["vocab_size"], (B, T), generator=g)
    midi = torch.randint(40, 90, (B, T), generator=g)
    dur = torch.rand(B, T, generator=g) * 0.8 + 0.05
    slur = torch.randint(0, 2, (B, T), generator=g)
    tok[B - 1, pad_from:] = 0
    return tok, midi, dur, slur


@functools.lru_cache(maxsize=None)
def decoder_input(T_mel, H, tail):
    """decoder_inp [1, T_mel, H] ~ N(0, 1) with its last `tail` frames zero, and the mel2ph (1 where live) that goes with it."""
    x = torch.randn(1, T_mel, H, generator=gen(820 + T_mel))
    m2p = torch.ones(1, T_mel, dtype=torch.long)
    if tail:
        x[:, T_mel - tail:] = 0.0
        m2p[:, T_mel - tail:] = 0
    return x, m2p


def bin_centres():
    """f0 (Hz, float64) at the centre of each of the 255 coarse bins on the mel scale: bin k is mel_k = mel_min + (k - 1) *
    span / 254."""
    k = torch.arange(1, 256, dtype=F64)
    mel = FP.F0_MEL_MIN + (k - 1.0) * (FP.F0_MEL_MAX - FP.F0_MEL_MIN) / (FP.F0_BIN - 2)
    return 700.0 * (torch.exp(mel / 1127.0) - 1.0)


def coarse_position(f0_hz, dtype=F64):
    """The real-valued bin position of f0 (before the + 0.5 and the truncation), in `dtype`."""
    m = 1127 * (1 + f0_hz.to(dtype) / 700).log()
    return (m - FP.F0_MEL_MIN) * (FP.F0_BIN - 2) / (FP.F0_MEL_MAX - FP.F0_MEL_MIN) + 1


EDGE_F0 = ((0.0, 1), (20.0, 1), (5000.0, 255), (-650.0, 1))          # Hz -> bin; f0 <= -700 Hz has no reference (log of <= 0)


@functools.lru_cache(maxsize=None)
def pitch_given_f0(B, T_mel, H):
    """origin [B, T_mel, H] (0 where mel2ph is 0), mel2ph, the caller's f0 [B, T_mel] in Hz (pitch_norm 'standard' with f0_mean 0
    and f0_std 1 hands it to f0_to_coarse as it is) at bin centres, cycling through all 255, with the EDGE_F0 values at the front
    of sample 0, and the bins they must land in (1 where mel2ph is 0)."""
    g = gen(830 + T_mel)
    origin = torch.randn(B, T_mel, H, generator=g)
    m2p = torch.randint(1, 200, (B, T_mel), generator=g)
    m2p[0, 40:52] = 0
    m2p[B - 1, T_mel - T_mel // 5:] = 0
    origin[m2p == 0] = 0.0
    hz = bin_centres()
    idx = (torch.arange(B * T_mel).reshape(B, T_mel) * 7) % 255
    f0_hz = hz[idx].clone()
    bins = idx + 1
    if T_mel > len(EDGE_F0):
        for i, (hz_i, bin_i) in enumerate(EDGE_F0):
            f0_hz[0, i], bins[0, i] = hz_i, bin_i
    bins = torch.where(m2p == 0, torch.ones_like(bins), bins)
    return origin, m2p, f0_hz.float(), bins


def pe_long_mel(B, T, M=80):
    """mel [B, T, M] uniform in [-5, 1) with zero frames 300 .. 339 and a zero tail (the last T / 10 frames of the last sample)."""
    mel = torch.rand(B, T, M, generator=gen(840 + T)) * 6.0 - 5.0
    mel[:, 300:340] = 0.0
    mel[B - 1, T - T // 10:] = 0.0
    return mel


def near_threshold(ref_pp, tol):
    """Frames whose reference voicing logit lies within tol * max|pitch_pred| of 0."""
    return ref_pp[..., 1].abs() <= tol * float(ref_pp.abs().max())


def conv_predictor_ref(sd, prefix, x, n_layers, k, table_init, dtype=F64):
    """PitchPredictor (tts_modules.py:247-260) without its mask: x [B, T, H] -> [B, T, n_out]."""
    dt = dtype
    w = lambda key: sd[prefix + key].to(dt)      # noqa: E731
    x = x.to(dt)
    T, H = x.shape[1], x.shape[2]
    tab = PE.sinusoid_table(max(table_init, T + 1), H).to(dt)
    x = x + w("pos_embed_alpha") * tab[PE.make_positions(x[..., 0])]
    x = x.transpose(1, 2)
    for i in range(n_layers):
        p = "conv.%d." % i
        x = F.relu(F.conv1d(F.pad(x, ((k - 1) // 2, (k - 1) // 2)), w(p + "1.weight"), w(p + "1.bias")))
        x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), w(p + "3.weight"), w(p + "3.bias"), EPS).transpose(1, 2)
    return F.linear(x.transpose(1, 2), w("linear.weight"), w("linear.bias"))
