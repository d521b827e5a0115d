"""The LDS-DMA engine's linear form and its compile-time epilogue kinds (csrc/igemm_dma.hip, csrc/igemm_epilogue.h: PLAIN, SPLIT,
GEGLU) against the kernel they replace: MAA_EPI=generic runs every launch on the convolution form with the generic epilogue.

Every case goes through maa_op_linear twice in one process, default and MAA_EPI=generic, and the two outputs must be equal bit
for bit.  The default one is also compared with an fp64 product at the operator tolerance of tests/test_gpu_ops.py (rel-max
2e-5); in the plain-bf16 mode the reference multiplies the operands rounded to bf16, as tests/test_gpu_bf16_engines.py does, so
that what is left is the fp32 summation order there too.

Shapes: the smallest at which each path can go wrong -- M a single ragged tile (1, 63), exact tiles (64, 128), a ragged last tile
of the 64- and the 128-row tiles (130, 250, 257); N below one tile (32: the 32-wide register tile, no variant), an exact tile (64,
128), a ragged N tile (96, 224), the model width (320); K one chunk (32), fewer chunks than stages (64), the model's K (320).
The tile of a launch is choose_tile's: with one context in flight these shapes all take 64x64, told that three are in flight
(set_concurrency(3)) M = 128 / 250 take 128x64 (N = 64, 320) and 128x128 (N = 128, 224), which the test asserts from the
profile rows, so all three instantiations run.  GEGLU always takes 128x128.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import check

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_gpu_ops.py

MS = [1, 63, 64, 128, 130, 250, 257]
NS = [32, 64, 96, 128, 224, 320]
KS = [32, 64, 320]
GEGLU_PACKED = [64, 128, 320, 640]


@pytest.fixture(scope="module", params=["bf16x3", "bf16"])
def ctx(request):
    from audiogpt_amd.backend import Context
    c = Context("cuda:0", precision=request.param)
    yield c
    c.close()


class forced:
    """The library parses the MAA_* knobs when a context is created; reload_tuning() re-reads them."""

    def __init__(self, **env):
        # the activation is handed over as split32 rows, as inside the models; the other engines that take linears stay out
        self.env = {"MAA_OP_PRESPLIT": "1", "MAA_PP": "off", "MAA_PP1": "off", "MAA_DMA2": "off"}
        self.env.update(env)

    def __enter__(self):
        from audiogpt_amd.backend import reload_tuning
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        reload_tuning()

    def __exit__(self, *a):
        from audiogpt_amd.backend import reload_tuning
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        reload_tuning()


def g(seed):
    return torch.Generator().manual_seed(seed)


def operand(t, precision):
    """What the mode multiplies, as float64: bf16x3 carries the fp32 operand, plain bf16 its rounding to bf16."""
    return (t.to(torch.bfloat16) if precision == "bf16" else t).to(torch.float64)


_cache = {}


def problem(precision, M, N, K):
    """Operands and the fp64 product of one shape, computed once and shared by every flag combination."""
    key = (precision, M, N, K)
    if key not in _cache:
        a = torch.randn(M, K, generator=g(1))
        w = torch.randn(N, K, generator=g(2)) / math.sqrt(K)
        b = torch.randn(N, generator=g(3))
        prod = torch.from_numpy(np.matmul(operand(a, precision).numpy(), operand(w, precision).numpy().T))
        _cache[key] = (a, w, b, prod)
    return _cache[key]


def unsplit(y):
    """split32 rows ([32 bf16 hi | 32 bf16 lo] per 32 columns, stored in the floats of an [M, N] tensor) -> float64 [M, N]."""
    M, N = y.shape
    h = y.cpu().contiguous().view(torch.bfloat16).reshape(M, N // 32, 2, 32).to(torch.float64)
    return (h[:, :, 0, :] + h[:, :, 1, :]).reshape(M, N)


def both(ctx, call):
    """call() under the default and under MAA_EPI=generic; asserts bit equality, returns the default's output."""
    with forced():
        y = call().cpu()
    with forced(MAA_EPI="generic"):
        y_gen = call().cpu()
    assert torch.equal(y.view(torch.int32), y_gen.view(torch.int32))
    return y


def tiles_seen(rows):
    """Tile indices (0 = 128x128, 1 = 128x64, 2 = 64x64) of the LDS-DMA launches in a detailed profile."""
    return {int(k[2]) for k in rows if k.startswith("bd")}


@pytest.mark.parametrize("concurrency", [1, 3])
@pytest.mark.parametrize("split_out", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_linear_default_equals_generic(ctx, bias, res, split_out, concurrency):
    ctx.set_concurrency(concurrency)
    ctx.prof_begin(detail=True)
    try:
        for M in MS:
            for N in NS:
                r = torch.randn(M, N, generator=g(4)) if res else None
                for K in KS:
                    a, w, b, prod = problem(ctx.precision, M, N, K)
                    y = both(ctx, lambda: ctx.op_linear(a, w, b if bias else None, res=r, split_out=split_out))
                    ref = prod + (b.double() if bias else 0.0) + (r.double() if res else 0.0)
                    check(f"variants_{ctx.precision}_c{concurrency}_{M}x{K}x{N}_b{int(bias)}r{int(res)}s{int(split_out)}",
                          unsplit(y) if split_out else y, ref, TOL)
    finally:
        rows = ctx.prof_end()
        ctx.set_concurrency(None)
    assert tiles_seen(rows) == ({0, 1, 2} if concurrency == 3 else {2}), sorted(rows)


@pytest.mark.parametrize("concurrency", [1, 3])
def test_geglu_default_equals_generic(ctx, concurrency):
    ctx.set_concurrency(concurrency)
    ctx.prof_begin(detail=True)
    try:
        for M in MS:
            for packed in GEGLU_PACKED:
                for K in KS:
                    a, w, b, prod = problem(ctx.precision, M, packed, K)
                    y = both(ctx, lambda: ctx.op_linear(a, w, b, geglu=True))
                    val, gate = (prod + b.double()).chunk(2, dim=-1)
                    check(f"variants_{ctx.precision}_c{concurrency}_geglu_{M}x{K}x{packed}", y, val * F.gelu(gate), TOL)
    finally:
        rows = ctx.prof_end()
        ctx.set_concurrency(None)
    assert tiles_seen(rows) == {0}, sorted(rows)


def test_a_convolution_keeps_the_generic_kernel(ctx):
    """A 3x3 convolution is not a linear: it runs the convolution form under either setting and returns what it returned."""
    B, Cin, Cout, H, W = 3, 64, 96, 7, 9
    x = torch.randn(B, Cin, H, W, generator=g(7))
    w = torch.randn(Cout, Cin, 3, 3, generator=g(8)) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g(9))
    ctx.prof_begin(detail=True)
    try:
        y = both(ctx, lambda: ctx.op_conv(x, w, b, pad=1))
    finally:
        rows = ctx.prof_end()
    assert tiles_seen(rows), sorted(rows)
    ref = F.conv2d(operand(x, ctx.precision), operand(w, ctx.precision), b.double(), padding=1)
    check(f"variants_{ctx.precision}_conv3x3", y, ref, TOL)
