"""Host-side yardstick for the row kernels of the Glow post-net run in reverse (csrc/glow.hip) and of the plain FastSpeech2
(csrc/fs2.hip) through maa_op_tts_rows: float64 references written from the formulas of the modules the kernels replace, and the
seeded input builders that tests/test_gpu_tts_ops.py and tests/test_tts_rows_ref.py share, so that the CPU test and the GPU test
see the same tensors.  Nothing here calls the library.

The Glow references work in the modules' own layout, [B, C, T] with x_mask [B, 1, T] (glow_modules.py: squeeze :742-755, ActNorm
:77-91, InvConvNear :147-182 with its own view / permute, CouplingBlock :320-332; wavenet.py:5-11 and :60-78); `rows_to_bct` /
`bct_to_rows` move between that and the kernels' channels-last rows.  Where tests/glow_ref.py or tests/fs2_plain_ref.py hold the
operation already (squeeze, the counted positions, the two position tables, the energy bin) theirs is used: those are held to
the goldens.

Every reference takes `dtype`: float64 is the yardstick, float32 is torch's own evaluation of the same formula, which
tests/test_tts_rows_ref.py holds to half of the gate the GPU test applies."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import fs2_plain_ref as FP
from tests import fs2_ref as FS
from tests import glow_ref as G
from tests import seq_ref as S

TOL_ROW = S.TOL_ROW            # rel-max against float64: elementwise work, LayerNorm
TOL_REDUCE = S.TOL_REDUCE      # ... where a reduction follows: the energy head's dot product, rowld
EPS = 1e-5
HUGE = 1.0e30
F32, F64 = torch.float32, torch.float64
gen = S.gen


def rows_to_bct(x, B=1):
    """[B * T, C] channels-last rows -> [B, C, T]."""
    return x.reshape(B, -1, x.shape[-1]).transpose(1, 2)


def bct_to_rows(x):
    """[B, C, T] -> [B * T, C]."""
    return x.transpose(1, 2).reshape(-1, x.shape[1])


def row_mask(rows):
    """[rows]: zeros at rows 2, 6, 10, ... and 0.5 at rows 1, 5, 9, ... (a single row: 1).  The modules multiply by x_mask after
    every stage, so a mask value that is neither 0 nor 1 shows each product: with 0 and 1 alone a dropped one changes nothing."""
    m = torch.ones(rows)
    m[2::4] = 0
    m[1::4] = 0.5
    return m


# ---------------------------------------------------------------------------------------------------- squeeze

SQ_C = (4, 20, 80, 132, 256)
SQ_T = (2, 3, 37, 40)
SQ_B = (1, 3)


def squeeze_lengths(T, B):
    """Live lengths of the ragged mask: the full length, T - 1 and about T / 2 made odd (one of the last two is odd whatever T is,
    so a pair with mask[2t'] = 1 and mask[2t' + 1] = 0 occurs); B = 1 takes the odd one of them."""
    half = max(T // 2, 1)
    full = [T, max(T - 1, 1), half if half % 2 else max(half - 1, 1)]
    return full if B == 3 else [n for n in full[1:] if n % 2][:1]


@functools.lru_cache(maxsize=None)
def squeeze_input(C, T, B, masked):
    """z [B, T, C] channels-last ~ N(0, 1) and mask [B, T] (None without): 1e30 on every frame behind the mask and on the live first
    frame of a pair the mask cuts; NaN on the odd last frame, which the kernel never reads."""
    z = torch.randn(B, T, C, generator=gen(1100 + C + T + B))
    mask = None
    if masked:
        mask = torch.zeros(B, T)
        for b, n in enumerate(squeeze_lengths(T, B)):
            mask[b, :n] = 1
            z[b, n:] = HUGE
            if n % 2:
                z[b, n - 1] = -HUGE
    if T % 2:
        z[:, T - 1] = float("nan")
    return z, mask


def squeeze_ref(z, mask, dtype=F64):
    """-> (rows [B * (T // 2), 2C], mask_s [B * (T // 2)]) by glow_ref.squeeze on [B, C, T]."""
    B, T, C = z.shape
    m = torch.ones(B, 1, T, dtype=dtype) if mask is None else mask.to(dtype)[:, None, :]
    xs, ms = G.squeeze(z.to(dtype).transpose(1, 2), m)
    return bct_to_rows(xs), ms.reshape(-1)


# ---------------------------------------------------------------------------------------------------- gate

GATE_H = (4, 32, 192, 260, 512)
GATE_ROWS = (1, 5, 9)
GATE_PLANTED = (100.0, -100.0, 88.0, -88.0, 30.0, -30.0, 0.0)


@functools.lru_cache(maxsize=None)
def gate_input(H, rows):
    """y [rows, 2H]: the tanh half uniform in [-2, 2], the sigmoid half uniform in [3, 12] with GATE_PLANTED going round both
    halves from column `row` on, in opposite orders (as many as the row holds) -- the two halves come from different ranges and
    the planted values never face themselves, so swapping the halves is no small change."""
    g = gen(1200 + H + rows)
    t = torch.rand(rows, H, generator=g) * 4.0 - 2.0
    s = torch.rand(rows, H, generator=g) * 9.0 + 3.0
    n = min(len(GATE_PLANTED), H)
    for r in range(rows):
        for i in range(n):
            s[r, (r + i) % H] = GATE_PLANTED[i]
            t[r, (r + i) % H] = GATE_PLANTED[n - 1 - i]
    return torch.cat([t, s], dim=1)


def gate_ref(y, dtype=F64):
    """fused_add_tanh_sigmoid_multiply after its add (wavenet.py:5-11), [B, 2H, T] inside."""
    x = rows_to_bct(y.to(dtype))
    H = x.shape[1] // 2
    return bct_to_rows(torch.tanh(x[:, :H]) * torch.sigmoid(x[:, H:]))


# ---------------------------------------------------------------------------------------------------- WN residual

WN_H = (4, 32, 192, 260, 512)
WN_ROWS = (1, 5, 9)


@functools.lru_cache(maxsize=None)
def wn_input(H, rows):
    """x [rows, H] (1e30 on the masked rows), rs of a first and a middle layer [rows, 2H] each and of a last layer [rows, H], mask."""
    g = gen(1300 + H + rows)
    x = torch.randn(rows, H, generator=g)
    rs = [torch.randn(rows, 2 * H, generator=g), torch.randn(rows, 2 * H, generator=g), torch.randn(rows, H, generator=g)]
    mask = row_mask(rows)
    x[mask == 0, ::3] = HUGE
    return x, rs, mask


def wn_step_ref(x, skip, rs, mask, first, last, dtype=F64):
    """One pass of WN's loop body after res_skip_layers[i] (wavenet.py:72-78), rows in, rows out -> (x, skip); `output * x_mask`
    belongs to the last layer.  skip is None on the first."""
    H = x.shape[1]
    m = mask.to(dtype)[None, None, :]
    xb, r = rows_to_bct(x.to(dtype)), rows_to_bct(rs.to(dtype))
    out = torch.zeros_like(xb) if first else rows_to_bct(skip.to(dtype))
    if not last:
        xb = (xb + r[:, :H]) * m
        out = out + r[:, H:]
    else:
        out = (out + r) * m
    return bct_to_rows(xb), bct_to_rows(out)


# ---------------------------------------------------------------------------------------------------- block tail

BT_C = (4, 8, 80, 132, 260, 512)
BT_ROWS = 9
# non-symmetric, diagonally dominant: condition number about 3, every off-diagonal pair (i, j) / (j, i) differs
BT_WINV = ((1.10, 0.35, -0.20, 0.15), (-0.30, 0.95, 0.40, -0.10), (0.25, -0.45, 1.20, 0.30), (-0.15, 0.20, -0.35, 0.90))


@functools.lru_cache(maxsize=None)
def bt_input(C, sigmoid_scale):
    """x, eo [rows, 2C], mask [rows], winv [4, 4], ActNorm bias and exp(-logs) [2C] (the exponential taken in float64 and rounded
    once, as the host hands it over), planted rowld [rows].  A masked row of x is zero in its first half and holds 1e30 in its
    second.  The raw scale lies in [-3, 3], under sigmoid_scale in [-14, 8], both ends planted in every row."""
    g = gen(1400 + C + sigmoid_scale)
    rows = BT_ROWS
    x = torch.randn(rows, 2 * C, generator=g)
    lo, hi = (-14.0, 8.0) if sigmoid_scale else (-3.0, 3.0)
    logs = torch.rand(rows, C, generator=g) * (hi - lo) + lo
    for r in range(rows):
        logs[r, r % C], logs[r, (r + C // 2) % C], logs[r, C - 1 - (r % 2)] = lo, hi, (lo if r % 3 else hi)
    eo = torch.cat([torch.randn(rows, C, generator=g), logs], dim=1)
    mask = row_mask(rows)
    x[mask == 0] = 0.0          # a block's input is masked already: the coupling hands x0 on as it is
    x[mask == 0, C + 1::5] = HUGE
    an_bias = 0.5 * torch.randn(2 * C, generator=g)
    an_logs = torch.rand(2 * C, generator=g) * 2.0 - 1.0
    an_einv = torch.exp(-an_logs.double()).float()
    rowld = torch.randn(rows, generator=g) * 10.0
    return x, eo, mask, torch.tensor(BT_WINV), an_bias, an_einv, rowld


def bt_ref(x, eo, mask, winv, an_bias, an_einv, sigmoid_scale, dtype=F64):
    """-> (h_cpl, h_inv, h_act [rows, 2C], ld [rows]): CouplingBlock's reverse after `end` (glow_modules.py:320-332), InvConvNear
    with the inverse weight handed over (:147-182, its own view / permute and conv2d), ActNorm in reverse (:77-91) with exp(-logs)
    handed over; ld is the coupling's -logs * x_mask summed over the channels only, the row's share of its logdet."""
    X, EO = rows_to_bct(x.to(dtype)), rows_to_bct(eo.to(dtype))
    b, c, t = X.shape
    C = c // 2
    m = mask.to(dtype)[None, None, :]
    x0, x1 = X[:, :C], X[:, C:]
    mu, logs = EO[:, :C], EO[:, C:]
    if sigmoid_scale:
        logs = torch.log(1e-6 + torch.sigmoid(logs + 2))
    z = torch.cat([x0, (x1 - mu) * torch.exp(-logs) * m], 1)
    ld = torch.sum(-logs * m, [1])[0]
    h_cpl = z
    n_split, n_sqz = 4, 2
    v = z.view(b, n_sqz, c // n_split, n_split // n_sqz, t)
    v = v.permute(0, 1, 3, 2, 4).contiguous().view(b, n_split, c // n_split, t)
    v = F.conv2d(v, winv.to(dtype).view(n_split, n_split, 1, 1))
    v = v.view(b, n_sqz, n_split // n_sqz, c // n_split, t)
    h_inv = v.permute(0, 1, 3, 2, 4).contiguous().view(b, c, t) * m
    h_act = (h_inv - an_bias.to(dtype)[None, :, None]) * an_einv.to(dtype)[None, :, None] * m
    return bct_to_rows(h_cpl), bct_to_rows(h_inv), bct_to_rows(h_act), ld


# ---------------------------------------------------------------------------------------------------- log-determinant sum

LD_TS = (1, 150, 256, 257, 700)
LD_B = (1, 3)
LD_PER_LEN = -3.7


@functools.lru_cache(maxsize=None)
def logdet_input(Ts, B):
    """rowld [B, Ts] of both signs, 0 behind the mask as the block tail leaves it; ragged mask [B, Ts]."""
    rowld = torch.randn(B, Ts, generator=gen(1500 + Ts + B)) * 50.0
    mask = torch.zeros(B, Ts)
    for b, n in enumerate((Ts, max(Ts - Ts // 3, 1), max(Ts // 4, 1))[:B]):
        mask[b, :n] = 1
    return rowld * mask, mask


def logdet_ref(rowld, mask, per_len):
    """The float64 sum of the fp32 rowld plus the fp32 per_len times the sample's length."""
    return rowld.double().sum(1) + torch.tensor(per_len, dtype=F32).double() * mask.double().sum(1)


def logdet_bound(rowld, mask, per_len):
    """The rounding bound of the kernel's fixed order: a thread's path to the result has ceil(Ts / 256) strided additions, 8 tree
    levels and the final multiply and add; each rounds once, by at most 2^-24 of a partial result that never exceeds the sum of
    the magnitudes."""
    Ts = rowld.shape[1]
    n_add = (Ts + 255) // 256 + 8 + 2
    return n_add * 2.0 ** -24 * (rowld.double().abs().sum(1) + abs(per_len) * mask.double().sum(1))


# ---------------------------------------------------------------------------------------------------- token positions, embedding

TP_T = (1, 33, 64, 65, 256, 257, 600)
TP_VOCAB = 11
EMB_H = (4, 256, 260, 384)
EMB_B, EMB_T, EMB_VOCAB = 2, 9, 13


@functools.lru_cache(maxsize=None)
def positions_tokens(T):
    """tok [3, T] int32: sample 0 with padding at the start (3 tokens) and single padding tokens inside; sample 1 with tokens
    64 .. 127 (a whole wave) and 256 .. 511 (a whole round of 256) padding; sample 2 all padding."""
    tok = torch.randint(1, TP_VOCAB, (3, T), generator=gen(1600 + T), dtype=torch.int32)
    tok[0, :3] = 0
    tok[0, 7::11] = 0
    tok[1, 64:128] = 0
    tok[1, 256:512] = 0
    tok[2] = 0
    return tok


def positions_table(T, H=4):
    """[T + 1, H]: row p holds p in every channel, so the embedding's output is the position itself."""
    return torch.arange(T + 1, dtype=F32)[:, None].repeat(1, H)


def positions_loop(tok):
    out = torch.zeros(tok.shape, dtype=torch.long)
    for b in range(tok.shape[0]):
        n = 0
        for t in range(tok.shape[1]):
            if int(tok[b, t]) != 0:
                n += 1
                out[b, t] = n
    return out


@functools.lru_cache(maxsize=None)
def embed_input(H, rel):
    """tok [2, 9] int32 with a negative token, tokens at and past the vocabulary and padding inside; E [vocab, H]; the position
    table of the form (fs2_plain_ref's sinusoid rows, T + 1 of them, or its RelPositionalEncoding rows); scale = sqrt(H) in fp32."""
    g = gen(1700 + H + rel)
    tok = torch.randint(2, EMB_VOCAB, (EMB_B, EMB_T), generator=g, dtype=torch.int32)      # (id 1 is left free for the GPU test)
    tok[0, 2], tok[0, 5], tok[0, 6] = 0, -3, EMB_VOCAB
    tok[1, 0], tok[1, 4], tok[1, 8] = EMB_VOCAB + 7, 0, 0
    E = torch.randn(EMB_VOCAB, H, generator=g)
    pe = FP.rel_table(EMB_T, H) if rel else FP.sinusoid_table(EMB_T + 1, H)
    return tok, E, pe, float(torch.tensor(math.sqrt(H), dtype=F32))


def embed_ref(tok, E, pe, scale, rel, dtype=F64):
    """forward_embedding and FFTBlocks' first mask (tts_modules.py:365-375, 320) on clamped token ids -> (x [B * T, H], nonpad
    [B * T])."""
    tok = tok.long()
    live = (tok != 0).to(dtype)
    x = scale * E.to(dtype)[tok.clamp(0, E.shape[0] - 1)]
    if rel:
        x = x * scale + pe.to(dtype)[None, :tok.shape[1]]
    else:
        x = x + pe.to(dtype)[FP.positions(tok)]
    return (x * live[:, :, None]).reshape(-1, E.shape[1]), live.reshape(-1)


# ---------------------------------------------------------------------------------------------------- speakers

SPK_H = (4, 256, 260)
SPK_B, SPK_T = 3, 7
GATHER_B = (1, 3, 5)
GATHER_ROWS = 5


@functools.lru_cache(maxsize=None)
def add_speaker_input(H):
    """x [21, H], spk [3, H], mask [21] of 0, 1 and 0.5, mel2ph [21] int32 of 0 and positive values."""
    g = gen(1800 + H)
    rows = SPK_B * SPK_T
    x, spk = torch.randn(rows, H, generator=g), torch.randn(SPK_B, H, generator=g)
    mask = torch.tensor([1.0, 0.5, 0.0, 1.0, 1.0, 0.5, 0.0] * SPK_B)
    m2p = torch.randint(1, 40, (rows,), generator=g, dtype=torch.int32)
    m2p[1::5] = 0
    return x, spk, mask, m2p


def add_speaker_ref(x, spk, live, dtype=F64):
    """(x + spk[:, None, :]) * live (fs2.py:114, 125), live [rows] bool."""
    H = x.shape[1]
    v = x.to(dtype).reshape(SPK_B, SPK_T, H) + spk.to(dtype)[:, None, :]
    return v.reshape(-1, H) * live.to(dtype)[:, None]


@functools.lru_cache(maxsize=None)
def gather_input(H, B):
    """Three distinct tables [5, H] and ids [3, B] int32 with one id below 0 and one past the table."""
    g = gen(1900 + H + B)
    tabs = [torch.randn(GATHER_ROWS, H, generator=g) + 10.0 * k for k in range(3)]
    ids = torch.randint(0, GATHER_ROWS, (3, B), generator=g, dtype=torch.int32)
    ids[0, 0], ids[2, B - 1] = -2, GATHER_ROWS + 2
    if B > 1:
        ids[1, 0] = GATHER_ROWS
    return tabs, ids


def gather_ref(tabs, ids, split, B):
    """[3, B, H]: the embeddings of fs2.py:104-110 on clamped ids; ids None: row b of each table."""
    out = []
    for k in range(3):
        idx = torch.arange(B) if ids is None else ids[k if split else 0].long().clamp(0, GATHER_ROWS - 1)
        out.append(tabs[k][idx])
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------- energy tail

EN_C = (4, 256, 260, 512, 516, 1024)      # NR = 1, 2, 4: a full and a partial row each
EN_H = (4, 256, 260)
EN_B, EN_T = 3, 7
EN_K = 37


def energy_planted():
    """A caller's energy [21] and its bins: k / 64 exactly and one ulp either side, 255 / 64 and above, 0 and below, NaN."""
    k = torch.tensor(EN_K / 64.0, dtype=F32)
    up, down = torch.nextafter(k, torch.tensor(9.0)), torch.nextafter(k, torch.tensor(-9.0))
    top = torch.tensor(255.0 / 64.0, dtype=F32)
    vals = [k, up, down, top, torch.nextafter(top, torch.tensor(-9.0)), torch.tensor(4.5), torch.tensor(1.0e30), torch.tensor(0.0),
            torch.tensor(-0.25), torch.tensor(-1.0e30), torch.tensor(float("nan")), torch.tensor(1.0 / 64.0),
            torch.nextafter(torch.tensor(1.0 / 64.0), torch.tensor(-9.0)), torch.tensor(2.0), torch.tensor(1.999999)]
    bins = [EN_K, EN_K, EN_K - 1, 255, 254, 255, 255, 0, 0, 0, 0, 1, 0, 128, 127]
    rows = EN_B * EN_T
    more = torch.rand(rows - len(vals), generator=gen(2001)) * 4.0
    e = torch.cat([torch.stack(vals).float(), more])
    return e, torch.tensor(bins + torch.floor(more.double() * 64.0).long().tolist())


def energy_bin_ref(e):
    """clamp(e * 256 // 4, max = 255) (fs2.py:167) in float64 with the device's clamp at 0; NaN lands in bin 0."""
    q = torch.floor(e.double() * 256.0 / 4.0)
    return torch.where(torch.isnan(q), torch.zeros_like(q), q.clamp(0, 255)).long()


def energy_head_ref(x, gamma, beta, w, bias, dtype=F64):
    return S.head_ref(x, gamma, beta, w, bias, dtype)[:, 0]


def energy_margin(e):
    """How far 64 e must stay from an integer for the bin to be certain at the head's gate."""
    return 64.0 * TOL_REDUCE * float(e.abs().max())


def energy_clear(e):
    q = e.double() * 64.0
    return bool(((q - torch.round(q)).abs() >= energy_margin(e)).all())


def _energy_draw(C, seed):
    g = gen(seed)
    rows = EN_B * EN_T
    x = F.relu(torch.randn(rows, C, generator=g) + 0.3)          # non-negative, as after the convolution's ReLU
    x[1] = S.HEAD_CONST
    x[2, (3 * C) // 4] = S.HEAD_LARGE
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = torch.randn(1, C, generator=g) / math.sqrt(C)
    return x, gamma, beta, w, torch.tensor([1.5])


@functools.lru_cache(maxsize=None)
def energy_head_input(C):
    """(x [21, C], gamma, beta, w [1, C], bias) from the first seed of 2100 + C, + 1000, ... whose float64 prediction keeps 64 e at
    least 64 * TOL_REDUCE * max|e| from every integer, so that every frame's bin is certain."""
    for k in range(256):
        d = _energy_draw(C, 2100 + C + 1000 * k)
        if energy_clear(energy_head_ref(*d)):
            return d
    raise AssertionError("no seed clear of the bin edges")


@functools.lru_cache(maxsize=None)
def energy_rows_input(H):
    """acc [21, H], energy_embed [256, H], spk [3, H], mel2ph [21] int32 with zeros and negative values."""
    g = gen(2200 + H)
    rows = EN_B * EN_T
    acc, table, spk = torch.randn(rows, H, generator=g), torch.randn(256, H, generator=g), torch.randn(EN_B, H, generator=g)
    m2p = torch.randint(1, 40, (rows,), generator=g, dtype=torch.int32)
    m2p[3::6] = 0
    m2p[10] = -1
    return acc, table, spk, m2p


def energy_tail_ref(acc, bins, table, spk, m2p, dtype=F64):
    """(decoder_inp + energy_embed[bin] + spk) * (mel2ph > 0) (fs2.py:168-172, 132), summed in that order; bins / spk None: without."""
    H = acc.shape[1]
    v = acc.to(dtype)
    if bins is not None:
        v = v + table.to(dtype)[bins]
    if spk is not None:
        v = (v.reshape(EN_B, EN_T, H) + spk.to(dtype)[:, None, :]).reshape(-1, H)
    return v * (m2p > 0).to(dtype)[:, None]


# ---------------------------------------------------------------------------------------------------- tgt mask

TGT_ROWS = (1, 255, 256, 257)


def tgt_input(rows):
    return torch.randint(-3, 6, (rows,), generator=gen(2300 + rows), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------- model lengths

PLAIN_T = (300, 600)


def plain_cfg():
    """fs2_plain_b2_t33's configuration cut to one encoder and one decoder layer, with seeded weights and the golden's duration
    bias."""
    from audiogpt_amd import weights as WT
    cfg, sd0, _ = FP.load_case("fs2_plain_b2_t33")
    cfg = dict(cfg, enc_layers=1, dec_layers=1)
    sd = WT.make_fs2_plain_state_dict(cfg, seed=FP.SEED)
    sd["dur_predictor.linear.bias"] = sd0["dur_predictor.linear.bias"]
    return cfg, sd


@functools.lru_cache(maxsize=None)
def plain_tokens(T, vocab):
    """tok [2, T]: padding tokens inside both samples (a whole wave of sample 0), sample 1 padding from 0.9 T on."""
    tok = torch.randint(1, vocab, (2, T), generator=gen(2400 + T))
    tok[0, 64:128] = 0
    tok[0, 5::37] = 0
    tok[1, 11::53] = 0
    tok[1, T - T // 10:] = 0
    return tok


def plain_encode_ref(sd, cfg, tok, dtype=F64):
    """The plain FastSpeech2's encode: embed_ref, then fs2_ref's FFTBlocks and duration predictor -> (encoder_out, xs, dur)."""
    H = cfg["hidden_size"]
    T = tok.shape[1]
    pe = FP.rel_table(T, H) if cfg["rel_pos"] else FP.sinusoid_table(T + 1, H)
    x, _ = embed_ref(tok, sd["encoder.embed_tokens.weight"], pe, float(torch.tensor(math.sqrt(H), dtype=F32)), cfg["rel_pos"], dtype)
    pad = tok.eq(0)
    enc = FS.fft_blocks(sd, "encoder", x.reshape(tok.shape[0], T, H), pad, cfg["num_heads"], cfg["enc_layers"],
                        cfg["enc_ffn_kernel_size"], dtype)
    xs, dur = FS.durations(sd, cfg, enc, pad, dtype)
    return enc, xs, dur


GLOW_LONG_T = 601


def glow_long_case():
    """glow_narrow_b2_t300's configuration and weights with z [2, C, 601], a ragged mask (601 and 411 live frames) and its
    conditioning."""
    cfg, sd, g0 = G.load_case("glow_narrow_b2_t300")
    g = gen(2500)
    T = GLOW_LONG_T
    z = torch.randn(2, cfg["in_channels"], T, generator=g)
    mask = torch.ones(2, 1, T)
    mask[1, :, 411:] = 0
    cond = torch.randn(2, g0["g"].shape[1], T, generator=g) if "g" in g0.files else None
    return cfg, sd, z, mask, cond
