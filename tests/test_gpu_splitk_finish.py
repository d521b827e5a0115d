"""The split-K finish (splitk_reduce_kernel, igemm_dma2.hip) on the layers that take it in the models, with every operand the
models hand to its epilogue: bias, the time-embedding row add, a residual, split32 output.

Shapes are ONE or TWO samples of the UNet's own layers, so that the number of K slices S is the model's:
    conv 3x3 640 -> 640 at 5 x 39    M = 195 (one 256-row tile, 61 dead rows)   ping-pong engine, S = 4
    conv 3x3 320 -> 320 at 10 x 78   M = 780 (not a multiple of 256)            ping-pong engine, S = 2
    linear K = 2560 -> N = 640       M = 195                                    second LDS-DMA engine, S = 2
With two samples, M = 390 / 1560: row 195 (780) falls inside a 32-row block (195 = 6 * 32 + 3, 780 = 24 * 32 + 12), so one block
of the reduce adds two samples' time-embedding rows.  No model splits the K of a GEGLU projection (the default policies of
both engines keep S = 1 for it), so the value / gate form of the reduce has no case here; tests/test_gpu_pp.py and
tests/test_gpu_dma2.py force one with MAA_PP1 / MAA_DMA2.

Checks, in bf16x3 and in plain bf16:
  * against an fp64 host reference at the operator tolerances of tests/test_gpu_pp.py (bf16x3: rel-max 2e-4) and
    tests/test_gpu_precision.py (bf16: 5e-2 -- 8-bit operands, |error| ~ 2^-9 per product, random-sign accumulation);
  * a sample alone equals the sample inside a batch, bit for bit;
  * repeated runs are bit-identical;
  * split32 output equals the split of the plain output, bit for bit (hi = bf16(v), lo = bf16(v - hi)).
The reduce has ONE form, the loop over the slices: a form unrolled for S = 2 / 4 was measured slower in the benchmark's
arrangement and not kept (profiles/splitk_finish_ab.txt), so there is no second form to compare it with.
"""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests.util import check

pytestmark = pytest.mark.gpu

TOL = {"bf16x3": 2e-4, "bf16": 5e-2}
CONVS = {"640@5x39": (640, 5, 39, 4), "320@10x78": (320, 10, 78, 2)}      # channels, H, W, K slices
COMBOS = ["bias", "rowadd", "res", "split"]


@pytest.fixture(scope="module", params=["bf16x3", "bf16"])
def ctx(request):
    from audiogpt_amd.backend import Context, reload_tuning
    saved = os.environ.get("MAA_OP_PRESPLIT")
    os.environ["MAA_OP_PRESPLIT"] = "1"       # the op entry points hand the activation over as split32 rows, as inside the models
    reload_tuning()
    c = Context("cuda:0", precision=request.param)
    yield c
    c.close()
    if saved is None:
        os.environ.pop("MAA_OP_PRESPLIT", None)
    else:
        os.environ["MAA_OP_PRESPLIT"] = saved
    reload_tuning()


def g(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """Inputs (fp32) and the fp64 convolution + bias of two samples, computed once."""
    C, H, W, _ = CONVS[name]
    x = torch.randn(2, C, H, W, generator=g(11))
    w = torch.randn(C, C, 3, 3, generator=g(12)) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g(13))
    rowadd = torch.randn(2, C, generator=g(14))
    res = torch.randn(2, C, H, W, generator=g(15))
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    return x, w, b, rowadd, res, ref


@functools.lru_cache(maxsize=None)
def linear_case():
    a = torch.randn(390, 2560, generator=g(21))
    w = torch.randn(640, 2560, generator=g(22)) / math.sqrt(2560)
    b = torch.randn(640, generator=g(23))
    res = torch.randn(390, 640, generator=g(24))
    return a, w, b, res, F.linear(a.double(), w.double(), b.double())


def unsplit(raw):
    """[rows, N] floats holding split32 rows -> (hi, lo) bf16 tensors [rows, N]."""
    rows, N = raw.shape
    h = raw.cpu().contiguous().view(torch.bfloat16).reshape(rows, N // 32, 2, 32)
    return h[:, :, 0].reshape(rows, N), h[:, :, 1].reshape(rows, N)


def split_of(v):
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("name", list(CONVS))
def test_conv_finish(ctx, name, combo):
    x, w, b, rowadd, res, ref = conv_case(name)
    C, H, W, _ = CONVS[name]
    kw = {}
    if combo == "rowadd":
        kw["rowadd"] = rowadd
        ref = ref + rowadd.double()[:, :, None, None]
    elif combo == "res":
        kw["res"] = res
        ref = ref + res.double()
    elif combo == "split":
        kw["split_out"] = True

    def run(lo, hi):
        sub = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in kw.items()}
        return ctx.op_conv(x[lo:hi], w, b, pad=1, **sub).cpu()

    y2, y1 = run(0, 2), run(1, 2)
    assert torch.equal(y2, run(0, 2)), "two runs differ"
    assert torch.equal(y2[1:2], y1), "a sample's result depends on its batch"
    tag = f"splitk_finish_{ctx.precision}_conv_{name}_{combo}"
    if combo == "split":
        plain = ctx.op_conv(x, w, b, pad=1).cpu().permute(0, 2, 3, 1).reshape(-1, C)      # [B H W][C], as the split rows
        hi, lo = unsplit(y2.reshape(-1, C))
        ehi, elo = split_of(plain)
        assert same_bits(hi, ehi) and same_bits(lo, elo), "split32 output is not the split of the plain output"
        y2 = (hi.float() + lo.float()).reshape(2, H, W, C).permute(0, 3, 1, 2)
        check(tag, y2, ref, TOL[ctx.precision])      # (hi + lo keeps 16 bits of the value: 2^-17 relative)
    else:
        check(tag, y2, ref, TOL[ctx.precision])
        check(tag + "_alone", y1, ref[1:2], TOL[ctx.precision])


@pytest.mark.parametrize("combo", ["bias", "res", "split"])
def test_linear_finish(ctx, combo):
    a, w, b, res, ref = linear_case()
    kw = {}
    if combo == "res":
        kw["res"] = res
        ref = ref + res.double()
    elif combo == "split":
        kw["split_out"] = True

    def run(lo, hi):
        sub = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in kw.items()}
        return ctx.op_linear(a[lo:hi], w, b, **sub).cpu()

    y2, y1 = run(0, 390), run(195, 390)
    assert torch.equal(y2, run(0, 390)), "two runs differ"
    assert torch.equal(y2[195:], y1), "a row's result depends on the rows it was computed with"
    tag = f"splitk_finish_{ctx.precision}_linear_2560_640_{combo}"
    if combo == "split":
        hi, lo = unsplit(y1)
        ehi, elo = split_of(ctx.op_linear(a[195:], w, b).cpu())
        assert same_bits(hi, ehi) and same_bits(lo, elo), "split32 output is not the split of the plain output"
        check(tag, hi.float() + lo.float(), ref[195:], TOL[ctx.precision])
    else:
        check(tag, y1, ref[195:], TOL[ctx.precision])
        check(tag + "_m390", y2, ref, TOL[ctx.precision])


def test_the_cases_take_the_split_k_engines(ctx):
    """The rows the library's profiler reports for the cases above: the engine and S the models' layers get."""
    for name, (C, H, W, S) in CONVS.items():
        x, w, b, *_ = conv_case(name)
        ctx.prof_begin(detail=True)
        ctx.op_conv(x[1:2], w, b, pad=1)
        rows = ctx.prof_end()
        assert f"pp160 M{H * W} N{C} K{9 * C} S{S}" in rows, rows.keys()
    a, w, b, *_ = linear_case()
    ctx.prof_begin(detail=True)
    ctx.op_linear(a[195:], w, b)
    rows = ctx.prof_end()
    assert "b2 M195 N640 K2560 t1" in rows, rows.keys()
    # (that row carries no S: the plain row name says whether the launch was split, for M = 195 and for M = 390)
    for lo in (195, 0):
        ctx.prof_begin()
        ctx.op_linear(a[lo:], w, b)
        rows = ctx.prof_end()
        assert any(k.startswith("igemm_") and "splitK" in k for k in rows), rows.keys()
