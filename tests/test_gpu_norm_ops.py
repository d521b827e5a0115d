"""The normalisation kernels as the models call them (csrc/norm.hip through maa_op_groupnorm_ex / maa_op_layernorm_ex /
maa_op_split32, which forward every argument of the library's internal calls): two GroupNorm sources without a concatenation,
row pitches wider than the channel count, the split32 output and the raw split32 copy, every instantiation of the one-pass
kernel and the automatic two-launch fallback, statistics under inputs whose first element / first position / last element is
far from typical of its group, LayerNorm up to 2048 columns, and the split32 codec on its own -- each against a float64
reference on the CPU (tests/norm_ref.py).

Tolerances are the operator ones of test_gpu_ops.py, rel-max against float64: 2e-5 GroupNorm, 1e-5 LayerNorm.
tests/test_norm_ref.py shows on the CPU that torch's own fp32 kernels stay within half of them on every input used here.

GroupNorm inputs sit inside wider buffers whose spare columns hold a large finite sentinel, and every output has 8 spare
rows of a sentinel behind it, so that a load or store beside the rows shows up with every access still inside an allocation."""
import contextlib
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R
from tests.util import check, record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIG = 1.0e30            # spare columns of the input buffers
SENTINEL = -12345.0     # spare rows behind every output
PAD = 8
PATHS = ("fused", "two_launch")


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def ctx(request):
    from audiogpt_amd.backend import Context
    c = Context(DEV, precision=request.param)
    yield c
    c.close()


@contextlib.contextmanager
def gn_path(path):
    """two_launch: MAA_GN_TWO_PASS=1 (gn_stats_kernel + gn_apply_kernel everywhere); fused: the default dispatch.  The library
    parses the MAA_* knobs when a context is created; reload_tuning() re-reads them."""
    from audiogpt_amd.backend import reload_tuning
    assert path in PATHS
    if path == "two_launch":
        os.environ["MAA_GN_TWO_PASS"] = "1"
    try:
        reload_tuning()
        yield
    finally:
        os.environ.pop("MAA_GN_TWO_PASS", None)
        reload_tuning()


def tag(ctx, group, *parts):
    return "norm_%s_%s_%s" % (group, ctx.precision, "_".join(str(p) for p in parts))


def _padded(src, lead, trail):
    """[B, HW, C] -> (device buffer [B*HW, ld] with `lead` / `trail` sentinel columns round the data, view at the data, ld)"""
    B, HW, C = src.shape
    ld = lead + C + trail
    buf = torch.full((B * HW, ld), BIG, dtype=torch.float32)
    buf[:, lead:lead + C] = src.reshape(B * HW, C)
    buf = buf.to(DEV)
    return buf, buf.view(-1)[lead:], ld


def run_gn(ctx, sources, gamma, beta, eps, silu, out_split=0, raw=False, padded=True):
    """One maa_op_groupnorm_ex call.  sources: one or two channels-last CPU tensors [B, HW, C_i].  Returns (y, raw) on the CPU as
    [B, HW, C] fp32-typed tensors (split32 rows where asked for), after checking that the sentinel rows did not move."""
    B, HW, _ = sources[0].shape
    C = sum(s.shape[-1] for s in sources)
    args, keep = [], []
    for i, s in enumerate(sources):
        buf, view, ld = _padded(s, 4 + 4 * i, 8 - 4 * i) if padded else _padded(s, 0, 0)
        keep.append(buf)
        args += [view, ld, s.shape[-1]]
    if len(sources) == 1:
        args += [None, 0, 0]
    out = torch.full((B * HW + PAD, C), SENTINEL, dtype=torch.float32, device=DEV)
    rw = torch.full((B * HW + PAD, C), SENTINEL, dtype=torch.float32, device=DEV) if raw else None
    ctx.op_groupnorm_ex(*args, B, HW, R.GROUPS, gamma, beta, eps, silu, out, out_split=out_split, raw=rw)
    res = []
    for t in (out, rw):
        if t is None:
            res.append(None)
            continue
        t = t.cpu()
        assert torch.equal(t[B * HW:], torch.full((PAD, C), SENTINEL)), "store past the last output row"
        res.append(t[:B * HW].reshape(B, HW, C))
    return res


@functools.lru_cache(maxsize=None)
def gn_case(C, HW, eps, silu):
    x = R.gn_input(R.gn_batch(C, HW), C, HW)
    ga, be = R.gn_params(C)
    return x, ga, be, R.groupnorm_ref([x], R.GROUPS, ga, be, eps, silu)


def _check_split(ctx, name, sources, ga, be, eps, silu, y, ref):
    """out_split = 1 and the raw copy of the same call: the arithmetic is the same and only the store differs, so the words are
    those of split32_encode on the fp32 result / on the concatenated input, bit for bit."""
    B, HW, C = y.shape
    ys, raw = run_gn(ctx, sources, ga, be, eps, silu, out_split=1, raw=True)
    assert torch.equal(ys.reshape(B * HW, C).view(torch.int32), R.split32_encode(y.reshape(B * HW, C)).view(torch.int32)), name
    x = torch.cat(sources, dim=-1).reshape(B * HW, C)
    assert torch.equal(raw.reshape(B * HW, C).view(torch.int32), R.split32_encode(x).view(torch.int32)), name + " raw"
    check(name + "_split", R.split32_decode(ys.reshape(B * HW, C), B * HW, C).reshape(B, HW, C), ref, R.GN_TOL)
    # the raw copy next to an fp32 result is the same copy
    y2, raw2 = run_gn(ctx, sources, ga, be, eps, silu, out_split=0, raw=True)
    assert torch.equal(y2, y) and torch.equal(raw2, raw), name + " raw beside fp32"


# ---- a. one source inside a wider buffer, every kernel instantiation, both paths

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("C,HW", sorted(R.GN_SHAPES))
def test_groupnorm_one_source_wide_pitch(ctx, C, HW, path):
    with gn_path(path):
        for eps, silu in R.GN_VARIANTS:
            x, ga, be, ref = gn_case(C, HW, eps, silu)
            name = tag(ctx, "gn1", path, f"C{C}_HW{HW}_eps{eps:g}_silu{int(silu)}")
            y, _ = run_gn(ctx, [x], ga, be, eps, silu)
            check(name, y, ref, R.GN_TOL)
            if C % 32 == 0:
                _check_split(ctx, name, [x], ga, be, eps, silu, y, ref)


# ---- b. two sources; the same call on the materialised concatenation

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("C1,C2,HW", R.GN_SPLITS)
def test_groupnorm_two_sources(ctx, C1, C2, HW, path):
    C = C1 + C2
    with gn_path(path):
        for eps, silu in R.GN_VARIANTS[:2]:
            x, ga, be, ref = gn_case(C, HW, eps, silu)
            src = R.split_sources(x, C1)
            name = tag(ctx, "gn2", path, f"{C1}+{C2}_HW{HW}_eps{eps:g}_silu{int(silu)}")
            y, _ = run_gn(ctx, src, ga, be, eps, silu)
            check(name, y, ref, R.GN_TOL)
            # both calls read the same values in the same order: bit for bit, with and without the wide pitch
            one, _ = run_gn(ctx, [x], ga, be, eps, silu, padded=False)
            assert torch.equal(y, one), name + ": two sources differ from their concatenation"
            if C % 32 == 0:
                _check_split(ctx, name, src, ga, be, eps, silu, y, ref)


# ---- c. batch, repeat and path invariance

@pytest.mark.parametrize("C1,C2,HW", [(64, 32, 77), (1280, 640, 195), (320, 640, 1200), (1280, 1280, 50)])
def test_groupnorm_batch_repeat_and_path_invariance(ctx, C1, C2, HW):
    x, ga, be, ref = gn_case(C1 + C2, HW, 1e-5, True)
    src = R.split_sources(x, C1)
    got = {}
    for path in PATHS:
        with gn_path(path):
            y, _ = run_gn(ctx, src, ga, be, 1e-5, True)
            again, _ = run_gn(ctx, src, ga, be, 1e-5, True)
            assert torch.equal(y, again), path + ": a repeat call differs"
            b = x.shape[0] - 1
            alone, _ = run_gn(ctx, [s[b:b + 1].contiguous() for s in src], ga, be, 1e-5, True)
            assert torch.equal(alone, y[b:b + 1]), path + ": a sample alone differs from the sample in its batch"
            got[path] = y
    d = float((got["fused"].double() - got["two_launch"].double()).abs().max() / ref.abs().max())
    record(tag(ctx, "gn_paths", f"{C1}+{C2}_HW{HW}"), rel_max=d, tol=R.GN_TOL)
    assert d <= R.GN_TOL, d


# ---- d. statistics under hard inputs

@pytest.mark.parametrize("case", R.HARD_CASES)
@pytest.mark.parametrize("C1,C2,HW", R.HARD_SHAPES)
def test_groupnorm_statistics_under_hard_inputs(ctx, C1, C2, HW, case):
    """Planted elements far from typical of their group (tests/norm_ref.py hard_input) must not cost the other elements their
    accuracy: besides the whole tensor, the elements that were not planted are compared relative to their own maximum, so that
    one large output cannot hide an error in the rest of its group.  A constant group comes out as (SiLU of) beta: the variance
    is clamped at 0 and rstd = 1 / sqrt(eps) is finite; it is compared at the tolerance and not bit for bit, because
    shift = beta - mean scale is rounded at the size of scale = gamma / sqrt(eps), about 316 gamma.
    With the group's first element as the pivot of shifted one-pass sums (both kernels, before their statistics were made
    independent of it) the planted-first-element and whole-position-0 cases miss the bound; the figures of both versions are in
    profiles/gn_pivot_ab.txt."""
    x, keep = R.hard_input(C1, C2, HW, case)
    ga, be = R.gn_params(C1 + C2)
    ref = _hard_ref(C1, C2, HW, case)
    src = R.split_sources(x, C1)
    for path in PATHS:
        with gn_path(path):
            name = tag(ctx, "gn_hard", path, f"{C1}+{C2}_HW{HW}_{case}")
            y, _ = run_gn(ctx, src, ga, be, 1e-5, True)
            one, _ = run_gn(ctx, [x], ga, be, 1e-5, True)
        assert torch.isfinite(y).all(), name
        assert torch.equal(y, one), name + ": two sources differ from their concatenation"
        failures = []
        for suffix, m in (("", None), ("_rest", keep)):
            a, b = (y, ref) if m is None else (y[m], ref[m])
            try:
                check(name + suffix, a, b, R.GN_TOL)
            except AssertionError as e:        # measure every figure of the case before failing
                failures.append(str(e))
        if case == "constant":
            c = R.constant_group_slice(C1, C2)
            want = F.silu(be.double())[c].expand_as(ref[..., c])
            err = float((y[..., c].double() - want).abs().max() / ref.abs().max())
            record(name + "_group", rel_max=err, tol=R.GN_TOL)
            if err > R.GN_TOL:
                failures.append(f"{name}_group: {err:.3e}")
        assert not failures, failures


@functools.lru_cache(maxsize=None)
def _hard_ref(C1, C2, HW, case):
    x, _ = R.hard_input(C1, C2, HW, case)
    ga, be = R.gn_params(C1 + C2)
    return R.groupnorm_ref([x], R.GROUPS, ga, be, 1e-5, True)


# ---- e. arguments: a bad test argument is an error string, not a fault

def test_groupnorm_ex_refuses_bad_arguments(ctx):
    from audiogpt_amd._lib import MaaError
    x = torch.zeros(2 * 5, 64, device=DEV)
    out = torch.full((2 * 5, 64), SENTINEL, device=DEV)
    ga, be = R.gn_params(64)

    def call(x1=x, ld1=64, C1=64, x2=None, ld2=0, C2=0, groups=32, out_split=0, g=ga, b=be):
        ctx.op_groupnorm_ex(x1, ld1, C1, x2, ld2, C2, 2, 5, groups, g, b, 1e-5, False, out, out_split=out_split)

    for kw, word in ((dict(ld1=60), "strides"), (dict(C1=32, x2=x, ld2=16, C2=32), "strides"), (dict(C1=32, C2=32), "second source"),
                     (dict(groups=24), "channels"), (dict(C1=30, ld1=64, g=ga[:30], b=be[:30]), "channels"),
                     (dict(C1=16, ld1=64, groups=16, out_split=1, g=ga[:16], b=be[:16]), "32-channel"),
                     (dict(x1=x.view(-1)[1:], ld1=64), "aligned")):
        with pytest.raises(MaaError, match=word):
            call(**kw)
    assert bool((out == SENTINEL).all()), "a refused call wrote to its output"
    with pytest.raises(MaaError, match="32-channel"):
        ctx.op_layernorm_ex(torch.zeros(3, 48), torch.ones(48), torch.zeros(48), out_split=1)
    with pytest.raises(MaaError, match="32-channel"):
        ctx.op_split32(torch.zeros(3, 48))


# ---- f. LayerNorm

@pytest.mark.parametrize("rows,C", R.LN_SHAPES)
def test_layernorm_ex(ctx, rows, C):
    ga, be = R.ln_params(C)
    for kind in R.LN_KINDS:
        x, keep = R.ln_input(rows, C, kind)
        for eps in R.LN_EPS:
            ref = R.layernorm_ref(x, ga, be, eps)
            name = tag(ctx, "ln", f"{rows}x{C}_{kind}_eps{eps:g}")
            y = ctx.op_layernorm_ex(x, ga, be, eps).cpu()
            check(name, y, ref, R.LN_TOL)
            check(name + "_rest", y[keep], ref[keep], R.LN_TOL)
            assert torch.equal(y, ctx.op_layernorm(x, ga, be, eps).cpu()), name + ": the plain entry differs"
            if C % 32 == 0:
                ys = ctx.op_layernorm_ex(x, ga, be, eps, out_split=1).cpu()
                assert torch.equal(ys.view(torch.int32), R.split32_encode(y).view(torch.int32)), name + " split"
    one = ctx.op_layernorm_ex(x[rows - 1:], ga, be, 1e-5).cpu()
    assert torch.equal(one, ctx.op_layernorm_ex(x, ga, be, 1e-5).cpu()[rows - 1:]), "a row alone differs from the row in its batch"


# ---- g. the split32 codec on its own

@pytest.mark.parametrize("rows,C", R.PACK_SHAPES)
def test_split32_pack_and_unpack(ctx, rows, C):
    x = R.pack_input(rows, C)
    for slope in (1.0, 0.1):
        want = R.split32_encode(F.leaky_relu(x, slope) if slope != 1.0 else x)
        packed = ctx.op_split32(x, slope=slope)
        assert torch.equal(packed.cpu().view(torch.int32), want.view(torch.int32)), f"pack slope {slope}"
        back = ctx.op_split32(packed, unpack=True).cpu()
        lines = want.view(torch.bfloat16).reshape(rows, C // 32, 64).to(torch.float32)
        hi_plus_lo = (lines[:, :, :32] + lines[:, :, 32:]).reshape(rows, C)        # the fp32 sum split32_decode forms in float64
        assert torch.equal(back.view(torch.int32), hi_plus_lo.view(torch.int32)), f"unpack slope {slope}"
        assert torch.equal(back.double(), R.split32_decode(packed, rows, C)), f"unpack against split32_decode, slope {slope}"
