"""Host-side yardsticks for the attention operator tests: a float64 reference, a float64 emulation of the fused
kernel's DESIGN (what a correct kernel of that design may differ from the reference by), the split32 row codec,
and the seeded inputs that the GPU tests and the CPU check of their gates share.  Nothing here calls the library."""
import math

import torch

LOG2E = 1.4426950408889634

# operator gates, rel-max against float64 (tests/test_gpu_ops.py, tests/test_gpu_precision.py)
GATE = {"f32": 2e-5, "bf16x3": 2e-4, "bf16": 5e-2}
TERMS = {"bf16x3": 3, "bf16": 1}
FLASH_DH = (32, 40, 64, 80)     # head widths the fused kernel takes in the bf16 modes


def gate(precision, dh):
    return GATE[precision] * (5 if dh >= 256 and precision != "f32" else 1)


def _causal_mask(Nq, Nk):
    return torch.arange(Nk)[None, :] > torch.arange(Nq)[:, None]      # True = key hidden from the query


def attention_ref(q, k, v, heads, alpha, causal=False, return_scores=False):
    """softmax(alpha q k^T) v per head in float64.  q [B, Nq, heads, dh], k / v [B, Nk, heads, dh] -> [B, Nq, heads, dh]
    (and the masked logits [B, heads, Nq, Nk], in nats, on request)."""
    assert q.dim() == 4 and q.shape[2] == heads and k.shape[2] == heads and v.shape == k.shape, (q.shape, k.shape, v.shape)
    q, k, v = (t.detach().to("cpu", torch.float64).permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(q, k.transpose(-1, -2)) * float(alpha)
    if causal:
        assert q.shape[2] == k.shape[2]
        s = s.masked_fill(_causal_mask(q.shape[2], k.shape[2]), -math.inf)
    out = torch.matmul(torch.softmax(s, dim=-1), v).permute(0, 2, 1, 3).contiguous()
    return (out, s) if return_scores else out


def _bf16(x):
    """Round to bf16 (nearest even) through fp32, back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _f32(x):
    return x.to(torch.float32).to(torch.float64)


def _split(x, terms):
    hi = _bf16(x)
    return (hi, None) if terms == 1 else (hi, _bf16(_f32(x - hi)))


def _mm(a, b, terms):
    """a @ b with both operands rounded to bf16 (terms = 1) or to bf16 hi + lo with the lo . lo product dropped (terms = 3);
    the sum itself is exact here (the kernel's fp32 accumulation is far below either rounding)."""
    ah, al = _split(a, terms)
    bh, bl = _split(b, terms)
    y = torch.matmul(ah, bh)
    if terms == 3:
        y = y + torch.matmul(ah, bl) + torch.matmul(al, bh)
    return y


def attention_emulated(q, k, v, alpha, terms, causal=False):
    """Float64 emulation of the fused kernel's design: scale . log2 e folded into Q in fp32 before the operands are rounded,
    fp32 scores in log2 units, softmax weights 2^(s - max) rounded like the operands before P . V, the row sum taken from the
    unrounded weights.  Same shapes as attention_ref."""
    assert terms in (1, 3)
    q, k, v = (t.detach().to("cpu", torch.float32).permute(0, 2, 1, 3) for t in (q, k, v))
    qs = (q * (torch.tensor(float(alpha), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))).to(torch.float64)
    k, v = k.to(torch.float64), v.to(torch.float64)
    s = _f32(_mm(qs, k.transpose(-1, -2), terms))
    if causal:
        s = s.masked_fill(_causal_mask(s.shape[-2], s.shape[-1]), -math.inf)
    p = _f32(torch.exp2(s - s.max(dim=-1, keepdim=True).values))
    o = _mm(p, v, terms) / p.sum(dim=-1, keepdim=True)
    return _f32(o).permute(0, 2, 1, 3).contiguous()


# ---- split32 rows: every 32 columns of a row take one 128-byte line [32 bf16 hi | 32 bf16 lo]; the row pitch stays that of fp32

def split32_encode(x, ld=None):
    """fp32 [rows, C] (C % 32 == 0) -> fp32-typed buffer [rows, ld] whose first C floats per row hold the split32 lines
    (hi = bf16(v), lo = bf16(v - hi)); columns C .. ld keep zeros."""
    rows, C = x.shape
    assert C % 32 == 0
    ld = C if ld is None else ld
    x = x.detach().to("cpu", torch.float32)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    lines = torch.cat([hi.reshape(rows, C // 32, 32), lo.reshape(rows, C // 32, 32)], dim=2)      # [rows, C/32, 64] bf16
    buf = torch.zeros(rows, ld, dtype=torch.float32)
    buf[:, :C] = lines.reshape(rows, 2 * C).contiguous().view(torch.float32)
    return buf


def split32_decode(buf, rows, C):
    """fp32-typed buffer holding split32 rows (row pitch = buf.shape[-1] floats) -> float64 [rows, C] = hi + lo."""
    assert C % 32 == 0
    buf = buf.detach().to("cpu").contiguous()
    assert buf.dtype == torch.float32
    buf = buf.reshape(-1, buf.shape[-1])
    assert buf.shape[0] >= rows and buf.shape[1] >= C, (buf.shape, rows, C)
    lines = buf[:rows, :C].contiguous().view(torch.bfloat16).reshape(rows, C // 32, 64).to(torch.float64)
    return (lines[:, :, :32] + lines[:, :, 32:]).reshape(rows, C)


# ---- seeded inputs shared by the GPU tests and the CPU check of their gates

def gen(seed):
    return torch.Generator().manual_seed(seed)


def random_qkv(B, heads, dh, Nq, Nk, seed, qscale=1.0, distinct_heads=False):
    """q, k, v ~ N(0, 1) as [B, N, heads, dh] fp32.  distinct_heads: q of head h scaled by (1 + h/4) and v of head h offset by
    +h, so that reading a neighbouring head's columns is an O(1) error."""
    q = torch.randn(B, Nq, heads, dh, generator=gen(seed)) * qscale
    k = torch.randn(B, Nk, heads, dh, generator=gen(seed + 1))
    v = torch.randn(B, Nk, heads, dh, generator=gen(seed + 2))
    if distinct_heads:
        h = torch.arange(heads, dtype=torch.float32)[None, None, :, None]
        q = q * (1.0 + h / 4.0)
        v = v + h
    return q, k, v


def far_apart_v(B, heads, dh, L, seed):
    """v whose row j has mean j: admitting or dropping one key moves the output by about 1 / (number of keys seen)."""
    return torch.randn(B, L, heads, dh, generator=gen(seed)) * 0.25 + torch.arange(L, dtype=torch.float32)[None, :, None, None]


CAUSAL_KINDS = ("random", "next")
CAUSAL_NATS = 20.0


def causal_qkv(B, heads, dh, L, alpha, kind, seed):
    """Inputs that make the causal edge visible at every row, not only where few keys are seen:
    random  q, k ~ N(0, 1), v row j has mean j: a near-uniform softmax, where dropping key i is an O(1) error of row 0 but
            admitting key i + 1 moves row i by 1 / (i + 2) only (3.7e-2 of the tensor's range at L = 200: under the bf16 gate);
    next    query i points with a 20-nat logit at key i + 1, the FIRST key it may not see, and v rows alternate in sign:
            admitting key i + 1, or dropping key i, is an error of the size of the tensor's range at every row."""
    if kind == "random":
        q, k, _ = random_qkv(B, heads, dh, L, L, seed)
        return q, k, far_apart_v(B, heads, dh, L, seed + 2)
    c = math.sqrt(CAUSAL_NATS / alpha)
    u = torch.randn(B, L, heads, dh, generator=gen(seed), dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    i = torch.arange(L)
    assert kind == "next"
    t = (i + 1).clamp_max(L - 1)
    sign = (1.0 - 2.0 * (i % 2)).to(torch.float32)[None, :, None, None]
    v = sign * (1.0 + i.to(torch.float32)[None, :, None, None] / L) + 0.25 * torch.randn(B, L, heads, dh, generator=gen(seed + 1))
    return (c * u[:, t]).to(torch.float32), (c * u).to(torch.float32), v


ONE_HOT_MAPS = ("ascending", "descending", "scatter")
ONE_HOT_NATS = 160.0


def one_hot_map(name, Nq, Nk):
    i = torch.arange(Nq)
    if name == "ascending":
        return i * Nk // Nq
    if name == "descending":
        return Nk - 1 - i * Nk // Nq
    assert name == "scatter"
    return (37 * i + 5) % Nk


def one_hot_qkv(B, heads, dh, Nq, Nk, alpha, name, seed):
    """Keys are random unit vectors times c, query i is c times the direction of key j(i), alpha c^2 = 160 nats: the softmax
    is one-hot and the exact answer is v[j(i)].  Returns q, k, v and j."""
    c = math.sqrt(ONE_HOT_NATS / alpha)
    u = torch.randn(B, Nk, heads, dh, generator=gen(seed), dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    j = one_hot_map(name, Nq, Nk)
    k = (c * u).to(torch.float32)
    q = (c * u[:, j]).to(torch.float32)
    v = torch.randn(B, Nk, heads, dh, generator=gen(seed + 1))
    return q, k, v, j


def one_hot_margin(scores, j):
    """Smallest gap, in nats, between the logit of key j(i) and the best other key of query i (inf with a single key)."""
    if scores.shape[-1] == 1:
        return math.inf
    idx = j.reshape(1, 1, -1, 1).expand(scores.shape[0], scores.shape[1], -1, 1)
    win = scores.gather(-1, idx)
    rest = scores.scatter(-1, idx, -math.inf).max(dim=-1, keepdim=True).values
    return float((win - rest).min())


ONE_HOT_SHAPES = ((780, 780), (1060, 1060), (195, 77), (300, 33), (257, 1))
ONE_HOT_MIN_MARGIN = 30.0       # nats; above it the answer does not depend on how the scores were rounded
SHARP_SHAPES = ((780, 780), (195, 77), (1060, 1060))
SHARP_SCALES = (2.0, 3.0, 4.0)
SHARP_CAUSAL_L = 200


def rel_max(a, b):
    a, b = a.to(torch.float64), b.to(torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
