"""Host-side yardsticks for the normalisation operator tests: float64 GroupNorm (over a list of channels-last sources, with
optional SiLU) and LayerNorm, a restatement of the fused GroupNorm's layout plan (which kernel a shape reaches), and the seeded
inputs that the GPU tests and the CPU check of their tolerances share.  Nothing here calls the library.  The split32 row codec
is tests/attn_ref.py's."""
import functools

import torch

from tests.attn_ref import gen, split32_decode, split32_encode      # noqa: F401  (re-exported for the tests)

GN_TOL = 2e-5       # rel-max against float64: tests/test_gpu_ops.py test_groupnorm
LN_TOL = 1e-5       # tests/test_gpu_ops.py test_layernorm
GROUPS = 32
SIGMA = 1.7         # spread of the Gaussian inputs; the planted elements are multiples of it


# ---- references

def groupnorm_ref(sources, groups, gamma, beta, eps, silu=False):
    """float64 GroupNorm of cat(sources, -1): sources are channels-last [B, HW, C_i]; gamma / beta [sum C_i] -> [B, HW, C]."""
    x = torch.cat([s.detach().to("cpu", torch.float64) for s in sources], dim=-1)
    B, HW, C = x.shape
    assert C % groups == 0
    g = x.reshape(B, HW, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(B, HW, C) * gamma.to(torch.float64) + beta.to(torch.float64)
    return y * torch.sigmoid(y) if silu else y


def layernorm_ref(x, gamma, beta, eps):
    """float64 LayerNorm over the last dim of x [rows, C]."""
    x = x.detach().to("cpu", torch.float64)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(torch.float64) + beta.to(torch.float64)


def rel_max(got, ref, mask=None):
    """max |got - ref| / max |ref|, both maxima over the elements where mask is True (all of them without a mask)."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    if mask is not None:
        got, ref = got[mask], ref[mask]
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ---- which kernel a GroupNorm shape reaches: csrc/norm.hip gn_fused_plan, restated

def fused_plan(C, HW, groups=GROUPS):
    """(gpb, nr, threads) of the one-pass kernel, or None where no plan fits and the statistics + apply launches run."""
    cpg = C // groups
    for cap in (8, 12, 16):
        for gpb in (4, 2, 8, 1, 16):
            if groups % gpb:
                continue
            CB = gpb * cpg
            if CB % 4 or CB > 512:
                continue
            Q = CB // 4
            RL = 1024 // Q
            if RL < 1:
                continue
            need = (HW + RL - 1) // RL
            if need > cap:
                continue
            nr = next(n for n in (1, 2, 4, 8, 12, 16) if need <= n)
            return gpb, nr, RL * Q
    return None


# (C, HW) -> what the shape reaches: (gpb, nr, threads) of the fused kernel, None = the automatic two-launch fallback
GN_SHAPES = {
    (96, 77): (4, 1, 1023),         # cpg 3: a float4 spans two groups
    (160, 331): (4, 2, 1020),       # cpg 5
    (640, 195): (4, 4, 1020),
    (1280, 195): (4, 8, 1000),
    (960, 780): (2, 12, 1020),
    (960, 1000): (2, 16, 1020),
    (960, 1200): None,              # cpg 30: 256 / 30 = 8 position lanes, 16 idle threads in gn_stats_kernel
    (2560, 50): (4, 8, 960),        # cpg 80, CB 320: 12 row lanes
    (32, 5): (4, 1, 1024),          # cpg 1, HW smaller than a row lane
}
# (C1, C2, HW): two sources.  A group straddles the boundary where C1 is no multiple of cpg (64|32, 96|64, 320|640, 1280|640); at
# the other splits the boundary falls between two groups of one workgroup's group block.
GN_SPLITS = ((64, 32, 77), (96, 64, 331), (320, 320, 195), (640, 640, 195), (320, 640, 780), (320, 640, 1000), (320, 640, 1200),
             (1280, 1280, 50), (1280, 640, 195), (12, 20, 5))
GN_VARIANTS = ((1e-5, True), (1e-6, False), (1e-6, True), (1e-5, False))       # (eps, silu)


def gn_batch(C, HW):
    return 3 if C * HW <= 300000 else 2


@functools.lru_cache(maxsize=None)
def gn_params(C, seed=0):
    """gamma, beta ~ N(0, 1), as tests/test_gpu_ops.py draws them."""
    return torch.randn(C, generator=gen(900 + seed)), torch.randn(C, generator=gen(901 + seed))


@functools.lru_cache(maxsize=None)
def gn_input(B, C, HW, seed=0):
    """Channels-last [B, HW, C] ~ N(0.3 + a per-channel offset, SIGMA^2): every channel and sample is distinct."""
    x = torch.randn(B, HW, C, generator=gen(910 + seed)) * SIGMA + 0.3
    return x + 0.5 * torch.randn(C, generator=gen(911 + seed))


def split_sources(x, C1):
    return [x[..., :C1].contiguous(), x[..., C1:].contiguous()] if 0 < C1 < x.shape[-1] else [x]


# ---- hard inputs for the statistics: each builder returns (x [B, HW, C], mask of the elements that were NOT planted)

HARD_SHAPES = ((64, 32, 77), (320, 640, 780), (1280, 640, 195), (320, 640, 1200), (1280, 1280, 50))
HARD_CASES = ("first100_x1", "first1000_x1", "first100_x2", "first1000_x2", "first100_straddle", "first1000_straddle",
              "pos0_50", "last100", "offset30", "constant")
CONSTANT = 0.75
HARD_B = 2


def hard_group(C1, C2, where):
    """Index of the group the case aims at: one that lies in x1, one that lies in x2, and the one that straddles the two
    buffers (where the boundary falls between two groups: the first group of x2, whose pivot-era first element was x2's)."""
    cpg = (C1 + C2) // GROUPS
    return {"x1": 1, "x2": GROUPS - 1, "straddle": C1 // cpg}[where]


@functools.lru_cache(maxsize=None)
def hard_input(C1, C2, HW, case):
    C = C1 + C2
    cpg = C // GROUPS
    x = gn_input(HARD_B, C, HW, seed=7).clone()
    keep = torch.ones_like(x, dtype=torch.bool)

    def plant(pos, ch, k):
        x[:, pos, ch] = k * SIGMA
        keep[:, pos, ch] = False

    if case.startswith("first"):
        k, where = case[5:].split("_")
        g = hard_group(C1, C2, where)
        assert (where == "x1" and (g + 1) * cpg <= C1) or (where == "x2" and g * cpg >= C1) or \
               (where == "straddle" and g * cpg <= C1 < (g + 1) * cpg)
        plant(0, g * cpg, float(k))
    elif case == "pos0_50":
        plant(0, slice(None), 50.0)
    elif case == "last100":
        plant(HW - 1, C - 1, 100.0)
    elif case == "offset30":
        x += 30.0 * SIGMA
    else:
        assert case == "constant"
        g = hard_group(C1, C2, "straddle")
        x[:, :, g * cpg:(g + 1) * cpg] = CONSTANT
    return x, keep


def constant_group_slice(C1, C2):
    cpg = (C1 + C2) // GROUPS
    g = hard_group(C1, C2, "straddle")
    return slice(g * cpg, (g + 1) * cpg)


# ---- LayerNorm

LN_SHAPES = ((33, 1280), (5, 2048), (9, 768), (7, 320), (1, 4), (1561, 640))
LN_EPS = (1e-5, 1e-12)      # ldm/modules/attention.py and config.py: CLIP / ViT-H towers 1e-5, BERT 1e-12
LN_KINDS = ("plain", "offset50", "spike1000")


@functools.lru_cache(maxsize=None)
def ln_params(C):
    return torch.randn(C, generator=gen(932)), torch.randn(C, generator=gen(933))


@functools.lru_cache(maxsize=None)
def ln_input(rows, C, kind):
    """plain: N(1, 3^2) as tests/test_gpu_ops.py; offset50: every row shifted by 50 sigma; spike1000: one element per row
    (column 37 r mod C) at 1000 sigma.  Returns (x, mask of the elements that were not planted).
    The offset is 50 sigma and not 100: at 100 sigma the rounding of the fp32 row mean alone (half an ulp of 300 is 0.5e-5
    sigma) puts torch's own fp32 layer_norm at 5.0e-6 of the float64 reference -- past half of LN_TOL at (33, 1280), (1, 4)
    and (1561, 640) -- so the input condition of tests/test_norm_ref.py shrinks it; the four-element row, whose own spread is
    that of four draws, misses it at 50 sigma too (6.3e-6) and takes 10 sigma."""
    x = torch.randn(rows, C, generator=gen(931)) * 3 + 1
    keep = torch.ones_like(x, dtype=torch.bool)
    if kind == "offset50":
        x = x + (150.0 if C >= 32 else 30.0)
    elif kind == "spike1000":
        r = torch.arange(rows)
        x[r, (37 * r) % C] = 3000.0
        keep[r, (37 * r) % C] = False
    else:
        assert kind == "plain"
    return x, keep


# ---- split32 codec

PACK_SHAPES = ((3, 32), (77, 96), (1000, 640))


@functools.lru_cache(maxsize=None)
def pack_input(rows, C):
    """N(0, 1) with the codec's edge values planted at the front: +-0, denormals, values exactly half way between two bf16
    (ties: to even, both directions, both signs), the largest finite bf16 and a value whose low half is itself a tie."""
    x = torch.randn(rows, C, generator=gen(940))
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00018000,
            0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f80ffff, 0x3f810001, 0x7f7f0000, 0xff7f0000,
            0x3f800080, 0x3f800180, 0x3f807f80, 0x3f808080, 0x3fffffff, 0x00800000, 0x80800000, 0x007f8000, 0x33800000]
    edge = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)
    flat = x.view(-1)
    n = min(edge.numel(), flat.numel())
    flat[:n] = edge[:n]
    flat[C - 1] = edge[3]         # the last column of a line
    return x
