"""The attention operator as the models call it (maa_op_attention_ex forwards every argument of the library's internal
attention call): the models' row layouts, causal masking, the split32 output, tile edges, and softmax inputs that force the
online-softmax branches of the fused kernel -- each against a float64 reference on the CPU (tests/attn_ref.py).

Gates are the operator tolerances of test_gpu_ops.py / test_gpu_precision.py, rel-max against float64: f32 2e-5, bf16x3 2e-4,
bf16 5e-2 (x 5 for dh >= 256 in the bf16 modes).  tests/test_attention_ref.py shows on the CPU that a float64 emulation of the
fused kernel's design stays within half of each gate on the inputs used here.

Every call goes through `run`: q / k / v sit in buffers with 32 spare rows of NaN after the last valid row and the output in
a buffer of a finite sentinel with 32 spare rows, so that an unmasked load shows up as a non-finite result and a stray store
as a changed sentinel, with every access still inside an allocation."""
import functools

import pytest
import torch

from tests import attn_ref as R
from tests.util import check, record

pytestmark = pytest.mark.gpu

PAD = 32                # spare rows behind every operand and behind the output
SENTINEL = -12345.0
ALL_DH = R.FLASH_DH + (48,)      # 48: a width the fused kernel does not take (GEMM + softmax + GEMM in every mode)


@pytest.fixture(scope="module", params=["f32", "bf16x3", "bf16"])
def ctx(request):
    from audiogpt_amd.backend import Context
    c = Context("cuda:0", precision=request.param)
    yield c
    c.close()


# ---- the four layouts: each helper returns {"q" | "k" | "v": (buffer [rows + PAD, ld], first column, ld, head stride)}

def _rows(t):
    B, N, H, dh = t.shape
    return t.reshape(B * N, H * dh)


def _buffer(rows, ld):
    return torch.full((rows + PAD, ld), float("nan"), dtype=torch.float32)


def pack_contiguous(q, k, v):
    """Three separate [B, N, heads*dh] tensors (maa_op_attention's convention)."""
    out = {}
    for name, t in (("q", q), ("k", k), ("v", v)):
        r = _rows(t)
        buf = _buffer(*r.shape)
        buf[:r.shape[0]] = r
        out[name] = (buf, 0, r.shape[1], t.shape[3])
    return out


def pack_fused(q, k, v):
    """Self-attention rows [q | k | v] of one projection, ld = 3 inner, head stride dh (unet.cpp attn1, the encoders' towers)."""
    assert q.shape == k.shape
    inner, dh = q.shape[2] * q.shape[3], q.shape[3]
    buf = _buffer(q.shape[0] * q.shape[1], 3 * inner)
    for i, t in enumerate((q, k, v)):
        buf[:-PAD, i * inner:(i + 1) * inner] = _rows(t)
    return {"q": (buf, 0, 3 * inner, dh), "k": (buf, inner, 3 * inner, dh), "v": (buf, 2 * inner, 3 * inner, dh)}


def pack_cross(q, k, v):
    """Cross-attention: q rows of pitch inner, k and v inside one [rows, 2 inner] buffer (unet.cpp attn2's K/V cache)."""
    inner, dh = q.shape[2] * q.shape[3], q.shape[3]
    bq = _buffer(q.shape[0] * q.shape[1], inner)
    bq[:-PAD] = _rows(q)
    bkv = _buffer(k.shape[0] * k.shape[1], 2 * inner)
    bkv[:-PAD, :inner] = _rows(k)
    bkv[:-PAD, inner:] = _rows(v)
    return {"q": (bq, 0, inner, dh), "k": (bkv, 0, 2 * inner, dh), "v": (bkv, inner, 2 * inner, dh)}


def pack_legacy(q, k, v):
    """Per-head [q | k | v] blocks, ld = 3 C, head stride 3 dh (QKVAttentionLegacy of the inpaint UNet)."""
    assert q.shape == k.shape
    B, N, H, dh = q.shape
    buf = _buffer(B * N, 3 * H * dh)
    buf[:-PAD] = torch.stack([q, k, v], dim=3).reshape(B * N, 3 * H * dh)
    return {"q": (buf, 0, 3 * H * dh, 3 * dh), "k": (buf, dh, 3 * H * dh, 3 * dh), "v": (buf, 2 * dh, 3 * H * dh, 3 * dh)}


PACK = {"contiguous": pack_contiguous, "fused": pack_fused, "cross": pack_cross, "legacy": pack_legacy}


def run(ctx, packed, B, heads, dh, Nq, Nk, alpha, causal=0, out_split=0, ldo=None, raw=False, refused=None):
    """One maa_op_attention_ex call on padded buffers.  Returns the output as [B, Nq, heads, dh] on the CPU (raw: the whole
    [B*Nq + PAD, ldo] buffer), after checking that no sentinel moved.  refused = a word of the expected error message: the
    call must raise it and write nothing."""
    C = heads * dh
    ldo = C if ldo is None else ldo
    dev, args = {}, []
    for name, N in (("q", Nq), ("k", Nk), ("v", Nk)):
        buf, col, ld, hs = packed[name]
        # the last element the library may read lies inside the valid rows of the buffer
        assert buf.shape == (B * N + PAD, ld) and col + (heads - 1) * hs + dh <= ld, (name, buf.shape, col, ld, hs)
        if id(buf) not in dev:
            dev[id(buf)] = buf.to("cuda:0")
        args += [dev[id(buf)].view(-1)[col:], ld, hs]
    assert ldo >= C
    out = torch.full((B * Nq + PAD, ldo), SENTINEL, dtype=torch.float32, device="cuda:0")
    if refused is not None:
        from audiogpt_amd._lib import MaaError
        with pytest.raises(MaaError, match=refused):
            ctx.op_attention_ex(*args, B, heads, dh, Nq, Nk, alpha, out, ldo, out_split=out_split, causal=causal)
        assert bool((out == SENTINEL).all()), "a refused call wrote to its output"
        return None
    ctx.op_attention_ex(*args, B, heads, dh, Nq, Nk, alpha, out, ldo, out_split=out_split, causal=causal)
    out = out.cpu()
    assert torch.equal(out[B * Nq:], torch.full((PAD, ldo), SENTINEL)), "store past the last output row"
    assert torch.equal(out[:, C:], torch.full((B * Nq + PAD, ldo - C), SENTINEL)), "store past the last output column"
    return out if raw else out[:B * Nq, :C].reshape(B, Nq, heads, dh)


def tag(ctx, group, *parts):
    return "attn_%s_%s_%s" % (group, ctx.precision, "_".join(str(p) for p in parts))


# ---- a. layouts

@functools.lru_cache(maxsize=None)
def layout_case(dh, cross):
    B, heads, Nq = 2, 3, 130
    Nk = 77 if cross else Nq
    q, k, v = R.random_qkv(B, heads, dh, Nq, Nk, seed=200 + dh, distinct_heads=True)
    return q, k, v, R.attention_ref(q, k, v, heads, dh ** -0.5)


@pytest.mark.parametrize("dh", ALL_DH)
@pytest.mark.parametrize("layout", ["contiguous", "fused", "cross", "legacy"])
def test_layouts(ctx, layout, dh):
    """Each model layout against float64, and against the contiguous layout of the same values bit for bit: neither the fused
    kernel's nor the GEMM path's arithmetic depends on pitches or head strides.  Head h of v is offset by +h and head h of q
    scaled by (1 + h/4): a neighbouring head's columns are an O(1) error."""
    q, k, v, ref = layout_case(dh, layout == "cross")
    B, Nq, heads, _ = q.shape
    a = (B, heads, dh, Nq, k.shape[1], dh ** -0.5)
    y = run(ctx, PACK[layout](q, k, v), *a)
    check(tag(ctx, "a", layout, "d%d" % dh), y, ref, R.gate(ctx.precision, dh))
    if layout != "contiguous":
        assert torch.equal(y, run(ctx, pack_contiguous(q, k, v), *a)), "layout changes the arithmetic"


# ---- b. poisoned padding (every test here runs on poisoned buffers; this one adds ldo > heads*dh and the single-head VAE form)

@pytest.mark.parametrize("layout,heads,dh,Nq,Nk,ldo_extra", [
    ("fused", 8, 40, 195, 195, 0), ("cross", 8, 40, 195, 77, 32), ("legacy", 4, 64, 265, 265, 8), ("cross", 2, 80, 33, 1, 4),
    ("fused", 2, 48, 130, 130, 16), ("fused", 1, 256, 100, 100, 32)])
def test_poisoned_padding(ctx, layout, heads, dh, Nq, Nk, ldo_extra):
    """NaN rows behind q / k / v, sentinel rows and columns behind the output: the result is finite and within tolerance and
    no sentinel moves (`run` asserts it with torch.equal).  Tail tiles of K / V and of the query rows read rows past Nk / Nq
    only if a mask is missing."""
    B = 2
    q, k, v = R.random_qkv(B, heads, dh, Nq, Nk, seed=300 + dh, distinct_heads=True)
    alpha = dh ** -0.5
    C = heads * dh
    y = run(ctx, PACK[layout](q, k, v), B, heads, dh, Nq, Nk, alpha, ldo=C + ldo_extra)
    check(tag(ctx, "b", layout, "h%d_d%d_%dx%d_ldo+%d" % (heads, dh, Nq, Nk, ldo_extra)), y,
          R.attention_ref(q, k, v, heads, alpha), R.gate(ctx.precision, dh))


# ---- c. tile edges: 128 query rows per workgroup, 32 per wave, 32 keys per tile

#  Nq: Nk                       every Nq of {1, 31, 32, 33, 127, 128, 129, 160, 161, 300} meets three Nk,
TILE_EDGES = {                # every Nk of {1, 2, 31, 32, 33, 63, 64, 65, 77, 257} meets three Nq
    1: (1, 32, 65),
    31: (2, 33, 77),
    32: (31, 63, 257),
    33: (32, 64, 1),
    127: (33, 65, 2),
    128: (63, 77, 31),
    129: (64, 257, 32),
    160: (65, 1, 33),
    161: (77, 2, 63),
    300: (257, 31, 64),
}


@functools.lru_cache(maxsize=None)
def edge_case(dh, Nq, Nk):
    q, k, v = R.random_qkv(2, 3, dh, Nq, Nk, seed=400 + dh, distinct_heads=True)
    return q, k, v, R.attention_ref(q, k, v, 3, dh ** -0.5)


@pytest.mark.parametrize("dh", [40, 64])
@pytest.mark.parametrize("Nq,Nk", [(nq, nk) for nq, nks in TILE_EDGES.items() for nk in nks])
def test_tile_edges(ctx, Nq, Nk, dh):
    q, k, v, ref = edge_case(dh, Nq, Nk)
    y = run(ctx, pack_cross(q, k, v), 2, 3, dh, Nq, Nk, dh ** -0.5)
    check(tag(ctx, "c", "d%d_%dx%d" % (dh, Nq, Nk)), y, ref, R.gate(ctx.precision, dh))


# ---- d. causal

@functools.lru_cache(maxsize=None)
def causal_case(dh, L, kind):
    alpha = dh ** -0.5
    q, k, v = R.causal_qkv(2, 2, dh, L, alpha, kind, seed=500 + dh)
    return q, k, v, R.attention_ref(q, k, v, 2, alpha, causal=True)


@pytest.mark.parametrize("kind", R.CAUSAL_KINDS)
@pytest.mark.parametrize("dh", [64, 80, 48])
@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 64, 77, 128, 129, 200])
def test_causal(ctx, L, dh, kind):
    """causal = 1 in the towers' fused layout: f32 (and dh = 48) take the softmax kernel's causal_nq, the bf16 modes the fused
    kernel's per-key mask.  Inputs: attn_ref.causal_qkv (the `next` kind turns one key too many or too few into an error of
    the tensor's range at every row).  Query 0 sees key 0 only: its output is v[0] to the precision of the mode."""
    q, k, v, ref = causal_case(dh, L, kind)
    y = run(ctx, pack_fused(q, k, v), 2, 2, dh, L, L, dh ** -0.5, causal=1)
    check(tag(ctx, "d", kind, "d%d_L%d" % (dh, L)), y, ref, R.gate(ctx.precision, dh))
    check(tag(ctx, "d", kind, "d%d_L%d_row0" % (dh, L)), y[:, 0], v[:, 0], R.gate(ctx.precision, dh))


@pytest.mark.parametrize("dh", [64, 48])
def test_causal_needs_square_scores(ctx, dh):
    """Nq != Nk with causal = 1 is an error, nothing is written, and the context works afterwards."""
    q, k, v = R.random_qkv(1, 2, dh, 40, 33, seed=7)
    run(ctx, pack_cross(q, k, v), 1, 2, dh, 40, 33, dh ** -0.5, causal=1, refused="causal")
    y = run(ctx, pack_cross(q, k, v), 1, 2, dh, 40, 33, dh ** -0.5)
    check(tag(ctx, "d", "after_error_d%d" % dh), y, R.attention_ref(q, k, v, 2, dh ** -0.5), R.gate(ctx.precision, dh))


# ---- e. key-slot probe: a one-hot softmax whose exact answer is v[j(i)]

@functools.lru_cache(maxsize=None)
def one_hot_case(dh, Nq, Nk, name):
    alpha = dh ** -0.5
    q, k, v, j = R.one_hot_qkv(1, 2, dh, Nq, Nk, alpha, name, seed=600 + dh)
    ref, scores = R.attention_ref(q, k, v, 2, alpha, return_scores=True)
    return q, k, v, j, ref, R.one_hot_margin(scores, j)


@pytest.mark.parametrize("name", R.ONE_HOT_MAPS)
@pytest.mark.parametrize("dh", ALL_DH)
@pytest.mark.parametrize("Nq,Nk", R.ONE_HOT_SHAPES)
def test_one_hot_key_slots(ctx, Nq, Nk, dh, name):
    """Query i points at key j(i) with a 160-nat logit (231 in the kernel's log2 units: 2^x without the running maximum
    overflows fp32), every other key is at least 30 nats behind, so the answer is v[j(i)] whatever the rounding of the scores.
    ascending / descending j: waves whose maximum moves in every tile up to the last, and waves that take the `no lane moved`
    skip from the second tile on; (37 i + 5) % Nk: every slot of a 32-key tile and both lane halves.  A wrong key-slot map, a
    V^T fragment that disagrees with it, a missing rescale or a stale maximum returns another row of v: an O(1) error."""
    q, k, v, j, ref, margin = one_hot_case(dh, Nq, Nk, name)
    assert margin >= R.ONE_HOT_MIN_MARGIN, margin
    exact = v[:, j]
    assert R.rel_max(ref, exact) < 1e-12
    y = run(ctx, pack_cross(q, k, v), 1, 2, dh, Nq, Nk, dh ** -0.5)
    check(tag(ctx, "e", name, "d%d_%dx%d" % (dh, Nq, Nk)), y, exact, R.gate(ctx.precision, dh))


# ---- f. sharp random softmax

@functools.lru_cache(maxsize=None)
def sharp_case(dh, Nq, Nk, scale, causal):
    q, k, v = R.random_qkv(1, 2, dh, Nq, Nk, seed=34, qscale=scale)
    return q, k, v, R.attention_ref(q, k, v, 2, dh ** -0.5, causal=causal)


@pytest.mark.parametrize("scale", R.SHARP_SCALES)
@pytest.mark.parametrize("dh", R.FLASH_DH)
@pytest.mark.parametrize("Nq,Nk,causal", [s + (False,) for s in R.SHARP_SHAPES] + [(R.SHARP_CAUSAL_L, R.SHARP_CAUSAL_L, True)])
def test_sharp_softmax(ctx, Nq, Nk, causal, dh, scale):
    """q ~ scale N(0, 1), scale 2 .. 4: logits up to about +-23 nats, so the running maximum keeps moving deep into the key
    loop and the rescale of O is taken with alpha well below 1."""
    q, k, v, ref = sharp_case(dh, Nq, Nk, scale, causal)
    pack = pack_fused if Nq == Nk else pack_cross
    y = run(ctx, pack(q, k, v), 1, 2, dh, Nq, Nk, dh ** -0.5, causal=int(causal))
    check(tag(ctx, "f", "x%g_d%d_%dx%d%s" % (scale, dh, Nq, Nk, "_causal" if causal else "")), y, ref,
          R.gate(ctx.precision, dh))


# ---- g. split32 output

@pytest.mark.parametrize("N", [129, 300])
@pytest.mark.parametrize("heads,dh", [(8, 40), (4, 64), (4, 80), (2, 32)])
def test_split_output(ctx, heads, dh, N):
    """out_split = 1 stores bf16 hi + lo of the very value out_split = 0 stores in fp32, so the decoded rows differ from the
    plain run by the hi + lo rounding alone: two 8-bit significands, |decoded - plain| <= 2^-16 |plain|; asserted with 2^-15.
    In f32 the fused kernel does not run and the library must refuse instead of writing."""
    B, C = 2, heads * dh
    q, k, v = R.random_qkv(B, heads, dh, N, N, seed=700 + dh, distinct_heads=True)
    a = (B, heads, dh, N, N, dh ** -0.5)
    if ctx.precision == "f32":
        run(ctx, pack_fused(q, k, v), *a, out_split=1, refused="split32")
        return
    plain = run(ctx, pack_fused(q, k, v), *a, ldo=C + 32).reshape(B * N, C).to(torch.float64)
    raw = run(ctx, pack_fused(q, k, v), *a, ldo=C + 32, out_split=1, raw=True)
    dec = R.split32_decode(raw, B * N, C)
    assert torch.isfinite(dec).all()
    err = float(((dec - plain).abs() / plain.abs().clamp_min(1e-30)).max())
    record(tag(ctx, "g", "h%d_d%d_N%d" % (heads, dh, N)), rel_max=err, tol=2.0 ** -15)
    assert bool(((dec - plain).abs() <= 2.0 ** -15 * plain.abs()).all()), err


def test_split_output_needs_the_fused_kernel(ctx):
    """dh = 48 is not a width of the fused kernel: out_split = 1 is the library's error in every mode, nothing is written and
    the context works afterwards."""
    B, heads, dh, N = 1, 2, 48, 40
    q, k, v = R.random_qkv(B, heads, dh, N, N, seed=8)
    run(ctx, pack_fused(q, k, v), B, heads, dh, N, N, dh ** -0.5, out_split=1, refused="split32")
    y = run(ctx, pack_fused(q, k, v), B, heads, dh, N, N, dh ** -0.5)
    check(tag(ctx, "g", "after_error_d48"), y, R.attention_ref(q, k, v, heads, dh ** -0.5), R.gate(ctx.precision, dh))


# ---- h. determinism, batch invariance, head permutation

@pytest.mark.parametrize("heads,dh,N", [(4, 32, 161), (4, 40, 195), (4, 64, 130), (4, 80, 195), (1, 512, 200)])
def test_determinism_and_invariance(ctx, heads, dh, N):
    """Bit for bit: two runs; sample b alone against sample b inside B = 3; permuted heads in, permuted heads out.  (The work
    of one (sample, head) does not depend on its neighbours: a workgroup of the fused kernel, a z-slice of the GEMMs.)"""
    B, alpha = 3, dh ** -0.5
    q, k, v = R.random_qkv(B, heads, dh, N, N, seed=800 + dh)
    y = run(ctx, pack_fused(q, k, v), B, heads, dh, N, N, alpha)
    check(tag(ctx, "h", "h%d_d%d_N%d" % (heads, dh, N)), y, R.attention_ref(q, k, v, heads, alpha), R.gate(ctx.precision, dh))
    assert torch.equal(y, run(ctx, pack_fused(q, k, v), B, heads, dh, N, N, alpha)), "two runs differ"
    for b in range(B):
        alone = run(ctx, pack_fused(q[b:b + 1], k[b:b + 1], v[b:b + 1]), 1, heads, dh, N, N, alpha)
        assert torch.equal(alone[0], y[b]), "sample %d depends on its batch" % b
    if heads > 1:
        perm = torch.tensor([2, 0, 3, 1])
        yp = run(ctx, pack_fused(q[:, :, perm], k[:, :, perm], v[:, :, perm]), B, heads, dh, N, N, alpha)
        assert torch.equal(yp, y[:, :, perm]), "a head depends on its position"
