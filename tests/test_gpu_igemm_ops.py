"""The contraction as the models issue it (csrc/igemm_*.hip and their shared epilogue csrc/igemm_epilogue.h, through
maa_op_igemm_ex = conv_into -> launch_igemm on device buffers laid out here): every field of the descriptor against the float64
restatement of tests/igemm_ref.py, on every engine, at the smallest shapes where the paths differ.  tests/test_igemm_ref.py shows
on the CPU that these inputs make each targeted mistake visible at the gates.

Gates (rel-max through tests.util.check, none new): f32 2e-5 (tests/test_gpu_ops.py), bf16x3 2e-4 (tests/test_gpu_pp.py), plain
bf16 2e-5 against a reference that rounds its operands (tests/test_gpu_linear_variants.py).  No gate is widened: the fp32 torch
restatement of the group (a) cases, tanh and erf-GELU included, is within 1.6e-6 of the reference (measured on the CPU by
tests/test_igemm_ref.py::test_the_fp32_restatement_is_well_inside_the_gates), so max(gate, 4 x that) is the gate.

Engines, forced as the existing operator files force them and asserted for EVERY call from its profile rows (detailed rows ig /
bg / bd / b2 / pp<bn> / pq<bn> with S<slices>; the second engine's slice count shows only in the plain row, `splitK`):
  F32        f32 context                                             BF16_REG   bf16 context, fp32 A; MAA_NO_DMA=1 with a split A
  DMA        presplit, MAA_PP=off MAA_PP1=off MAA_DMA2=off, and MAA_EPI=generic on the 1x1 cases (the linear form's other arm)
  DMA2       MAA_DMA2=0,4,1,1 and 0,4,1,2                            PP  MAA_PP=128,1 / 128,2 / 160,2 on the 3x3 cases
  PP1        MAA_PP1=128,1 / 128,2 / 160,2 on the 1x1 cases          (the `,2` variants finish in splitk_reduce_kernel, one
                                                                      geometry per engine: 128x128, 256x128, 256x160)
Shapes (tests/igemm_ref.py): B=3 5x7 -- 35 rows per sample, M = 105, so 32-row blocks straddle two samples at rows 35 and 70 (the
RSEL = true row add picks between two samples' rows inside a block) and every tile size has dead rows; B=5 3x5 -- 15 rows per
sample, RSEL = false (one division per row), a block spans three samples.  Cin = 64: 18 chunks for the 3x3, two for the 1x1, enough
for two K slices.  Cout 96 (split32-capable; ragged against 64-, 128- and 160-wide tiles), 78 (even: pair stores, ragged 32-column
block), 77 (odd: no pair stores).  3x3 "same" (convolution form) and 1x1 (the linear form of the LDS-DMA engine, which must fall to
Epi::GENERIC as soon as a term beyond bias / residual is present).

 (a) terms        alpha, bias, row add out of a [B, N+32] slab at column 32 (ld_rowadd != N), residual with ldr = N+8, act 1..4,
                  out_scale, accumulate, ldc = N+8 -- one at a time (each run-time branch of igemm_epilogue_impl alone), then all at
                  once with each activation in turn (the order ((acc alpha + bias + rowadd + res) -> act) out_scale + c).
 (b) store forms  PAIR / Epi::PLAIN need N even, ldc even and an 8-byte aligned base: N = 78 with ldc 78 / 80 (pair), 79 (odd
                  pitch), base + 1 float (4-byte aligned) with either pitch; N = 77 (odd) with ldc 77 / 78; N = 96 with and without c2
                  (c2 switches the pair form off; bf16 engines), each at both alignments.  On the DMA linear form default == MAA_EPI=generic, bits.
 (c) split32 out  N = 96: c_split with bias + res (Epi::SPLIT on the linear form, store_split_pair elsewhere), with erf-GELU and with
                  the row add (generic only); c2 beside an fp32 c with leaky.  Bits: the split output = split32 of the plain output of
                  the same call; c2 = split32 of leaky(c) of the same launch.  accumulate + c_split, a GEGLU with any further term, a
                  split32 output of N % 32 != 0 and any split32 output of the exact-fp32 engine are refused by igemm_plan.
 (d) GEGLU        M 1 / 63 / 130 / 257, packed N 128 / 320, K 32 / 320 (tests/test_gpu_linear_variants.py's), fp32 and split32 output
                  (M = 63 and 257 with ldc = N+8): Epi::GEGLU's c_split branch on DMA (both MAA_EPI arms, concurrency 1 and 3),
                  store_split_pair under p.geglu on PP1 and DMA2 with one and two slices.  K = 32 is one chunk: PP1 needs two
                  (igemm_pp1_takes, K >= 64) and hands it to DMA, DMA2 runs it as one slice -- asserted as such.
 (e) two sources  (64, 32) and (32, 96) with ld1 = C1+32: chunk 16 on F32, chunk 32 on BF16_REG (both bf16 modes); (9, 4) and (20, 12)
                  on F32's per-element gather; random weights and one-hot probes of every tap; one source with K = 77, ld1 = 80 and a
                  large finite fill in the three floats the aligned gather over-reads.
     A side       leaky-relu of A (staged from fp32, or packed into the split32 rows) and the virtual nearest-2x upsample of the
                  gather, on every engine that takes them.
 (f) outside      after EVERY call of this file: each float of c / c2 outside [M rows] x [N columns] -- pitch padding, the floats
                  in front of an offset base, three spare rows -- still holds the fill pattern (launch()).
 (g) contracts    on the all-terms case: two runs are bit-identical, a sample alone equals the sample in its batch; PP1 / DMA2 with
                  one slice == DMA == BF16_REG under MAA_NO_DMA, PP1 128,2 == DMA2 with two slices (tests/test_gpu_bf16_engines.py,
                  tests/test_gpu_pp.py and tests/test_gpu_dma2.py assert these for the plain form).
"""
import copy
import os

import pytest
import torch

from tests import igemm_ref as R
from tests.util import check

pytestmark = pytest.mark.gpu

BF = ("bf16x3", "bf16")
OFF = dict(MAA_PP="off", MAA_PP1="off", MAA_DMA2="off")
KNOBS = ("MAA_PP", "MAA_PP1", "MAA_DMA2", "MAA_NO_DMA", "MAA_EPI")

# row: prefix of the detailed profile row; S: K slices it must name; plain: assert from the plain rows instead
ENGINES = {
    "F32": dict(modes=("f32",), env={}, presplit=0, row="ig"),
    "BF16_REG": dict(modes=BF, env={}, presplit=0, row="bg"),
    "BF16_REG_split": dict(modes=BF, env={"MAA_NO_DMA": "1"}, presplit=1, row="bg"),
    "DMA": dict(modes=BF, env=OFF, presplit=1, row="bd"),
    "DMA_generic": dict(modes=BF, env=dict(OFF, MAA_EPI="generic"), presplit=1, row="bd", kernels=(1,)),
    "DMA2_s1": dict(modes=BF, env=dict(OFF, MAA_DMA2="0,4,1,1"), presplit=1, row="b2"),
    "DMA2_s2": dict(modes=BF, env=dict(OFF, MAA_DMA2="0,4,1,2"), presplit=1, row="igemm_dma2", plain=True, S=2),
    "PP_128_1": dict(modes=BF, env={"MAA_PP": "128,1"}, presplit=1, row="pp128", S=1, kernels=(3,)),
    "PP_128_2": dict(modes=BF, env={"MAA_PP": "128,2"}, presplit=1, row="pp128", S=2, kernels=(3,)),
    "PP_160_2": dict(modes=BF, env={"MAA_PP": "160,2"}, presplit=1, row="pp160", S=2, kernels=(3,)),
    "PP1_128_1": dict(modes=BF, env={"MAA_PP": "off", "MAA_PP1": "128,1"}, presplit=1, row="pq128", S=1, kernels=(1,)),
    "PP1_128_2": dict(modes=BF, env={"MAA_PP": "off", "MAA_PP1": "128,2"}, presplit=1, row="pq128", S=2, kernels=(1,)),
    "PP1_160_2": dict(modes=BF, env={"MAA_PP": "off", "MAA_PP1": "160,2"}, presplit=1, row="pq160", S=2, kernels=(1,)),
}
ON = [(e, p) for e, spec in ENGINES.items() for p in spec["modes"]]
ON_BF16 = [(e, p) for e, p in ON if p != "f32"]


@pytest.fixture(scope="module")
def ctxs():
    from audiogpt_amd.backend import Context
    cs = {p: Context("cuda:0", precision=p) for p in ("f32",) + BF}
    yield cs
    for c in cs.values():
        c.close()


class forced:
    """The library parses the MAA_* knobs when a context is created; reload_tuning() re-reads them.  Every knob that chooses an
    engine is set (empty = the default policy), so nothing leaks in from outside."""

    def __init__(self, engine=None, **env):
        self.env = {k: "" for k in KNOBS}
        if engine:
            self.env.update(ENGINES[engine]["env"])
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


def kernels_of(engine):
    return ENGINES[engine].get("kernels", R.KERNELS)


def launch(ctx, c, presplit=0, **extra):
    """One maa_op_igemm_ex call on fresh device copies of the case's buffers.  Returns (c, c2) as [M, N] fp32 CPU tensors (split32
    rows where asked for: the raw floats), after asserting (f): nothing outside [M] x [N] of either output changed."""
    dev = ctx.device
    up = lambda t: t.to(dev) if t is not None else None
    cbuf, c2buf = up(c.c), up(c.c2)
    c.call(ctx.op_igemm_ex, up(c.x1), up(c.x2), up(c.rowadd), up(c.res), cbuf[c.lead:], c2buf[c.lead:] if c2buf is not None else None,
           presplit=presplit, **extra)
    out = []
    for buf, ld in ((cbuf, c.ldc), (c2buf, c.ldc2)):
        if buf is None:
            out.append(None)
            continue
        host = buf.cpu()
        assert R.outside_untouched(host, c.M, c.N, ld, c.lead), "a float outside the result was written"
        out.append(R.rows_of(host[c.lead:], c.M, ld, c.N).clone())
    return out


def assert_engine(rows, engine, slices=None):
    spec = ENGINES[engine]
    S = spec.get("S") if slices is None else slices
    hit = [k for k in rows if k.startswith(spec["row"])]
    assert hit, (engine, sorted(rows))
    if spec.get("plain"):
        assert all(("splitK" in k) == (S > 1) for k in hit), (engine, S, hit)
    elif S is not None:
        assert all(k.endswith(" S%d" % S) for k in hit), (engine, S, hit)


def run(ctx, engine, c, slices=None, expect=None, **extra):
    """launch() on the engine (its knobs are already in force), asserting from this call's profile rows that it ran."""
    spec = ENGINES[engine]
    ctx.prof_begin(detail=not spec.get("plain"))
    try:
        y = launch(ctx, c, presplit=spec["presplit"], **extra)
    finally:
        rows = ctx.prof_end()
    assert_engine(rows, expect or engine, slices)
    return y


def bits(t):
    return t.contiguous().view(torch.int32)


def split_of(y):
    """[M, N] fp32 -> its split32 rows (hi = bf16(v), lo = bf16(v - hi)) as the floats an [M, N] tensor holds."""
    return R.split32_encode(y)


def value(c, y):
    return R.split32_decode(y, c.M, c.N) if c.kw["c_split"] else y


# ------------------------------------------------------------------------------------------------ (a) terms
@pytest.mark.parametrize("engine,precision", ON)
def test_terms_one_at_a_time_and_all_at_once(ctxs, engine, precision):
    ctx = ctxs[precision]
    with forced(engine):
        for name, c in R.term_cases(kernels=kernels_of(engine)):
            y, _ = run(ctx, engine, c)
            check(f"igemm_{engine}_{precision}_{name}", y, c.reference(precision)[0], R.GATE[precision])


# ------------------------------------------------------------------------------------------------ (b) store forms
def store_form_cases(kernels, second=True):
    for B, H, W in R.IMAGES:
        for k in kernels:
            for Cout, ldc_pad, lead, c2 in R.STORE_FORMS:
                if c2 and not second:
                    continue
                yield (f"b{B}_k{k}_n{Cout}_ldc{Cout + ldc_pad}_lead{lead}_c2{int(c2)}",
                       R.case(B=B, H=H, W=W, C1=R.CIN, Cout=Cout, k=k, bias=True, res=True, ldc_pad=ldc_pad, lead=lead, c2=c2, seed=12))


@pytest.mark.parametrize("engine,precision", ON)
def test_store_form_selection(ctxs, engine, precision):
    ctx = ctxs[precision]
    with forced(engine):
        for name, c in store_form_cases(kernels_of(engine), second=precision != "f32"):      # (the exact engine writes fp32 rows only)
            y, y2 = run(ctx, engine, c)
            ref, ref2 = c.reference(precision)
            check(f"igemm_store_{engine}_{precision}_{name}", y, ref, R.GATE[precision])
            if y2 is not None:
                check(f"igemm_store_c2_{engine}_{precision}_{name}", R.split32_decode(y2, c.M, c.N), ref2, R.GATE[precision])
                assert torch.equal(bits(y2), bits(split_of(R.leaky32(y, R.SLOPE)))), name


@pytest.mark.parametrize("precision", BF)
def test_dma_linear_form_equals_the_generic_arm(ctxs, precision):
    """The 1x1 cases of (a) and (b) on the LDS-DMA engine: linear form with its compile-time epilogue kind where one applies,
    against MAA_EPI=generic (convolution form, generic epilogue), bit for bit."""
    ctx = ctxs[precision]
    cases = list(R.term_cases(kernels=(1,))) + list(store_form_cases((1,)))
    with forced("DMA"):
        got = [launch(ctx, c, presplit=1) for _, c in cases]
    with forced("DMA_generic"):
        for (name, c), (y, y2) in zip(cases, got):
            g, g2 = launch(ctx, c, presplit=1)
            assert torch.equal(bits(y), bits(g)), name
            assert y2 is None or torch.equal(bits(y2), bits(g2)), name


# ------------------------------------------------------------------------------------------------ (c) split32 outputs
@pytest.mark.parametrize("engine,precision", ON_BF16)
def test_split32_outputs(ctxs, engine, precision):
    ctx = ctxs[precision]
    with forced(engine):
        for B, H, W in R.IMAGES:
            for k in kernels_of(engine):
                for tag, terms in R.SPLIT_OUTS.items():
                    name = f"{engine}_{precision}_{tag}_b{B}_k{k}"
                    c = R.case(B=B, H=H, W=W, C1=R.CIN, Cout=96, k=k, seed=13, **terms)
                    y, y2 = run(ctx, engine, c)
                    ref, ref2 = c.reference(precision)
                    check(f"igemm_split_{name}", value(c, y), ref, R.GATE[precision])
                    if c.kw["c_split"]:      # the same call with an fp32 output: same inputs (the seed), same engine
                        plain = R.case(B=B, H=H, W=W, C1=R.CIN, Cout=96, k=k, seed=13, **dict(terms, c_split=False))
                        yp, _ = run(ctx, engine, plain)
                        assert torch.equal(bits(y), bits(split_of(yp))), name
                    else:
                        check(f"igemm_split_c2_{name}", R.split32_decode(y2, c.M, c.N), ref2, R.GATE[precision])
                        assert torch.equal(bits(y2), bits(split_of(R.leaky32(y, R.SLOPE)))), name


@pytest.mark.parametrize("precision", ("f32",) + BF)
def test_what_the_epilogue_would_drop_is_refused(ctxs, precision):
    """igemm_plan refuses what the epilogue has no code for, instead of leaving the term out: accumulate onto a split32 output, a
    GEGLU with a residual / activation / output scale / accumulate, split32 lines of a width that is no multiple of 32, and on the
    exact-fp32 engine (whose own epilogue writes fp32 rows only) any split32 output."""
    from audiogpt_amd._lib import MaaError
    ctx = ctxs[precision]
    B, H, W = R.IMAGES[0]
    pre = int(precision != "f32")
    with forced("DMA"):
        c = R.Case(B=B, H=H, W=W, C1=R.CIN, Cout=96, bias=True, accumulate=True, c_split=True, seed=16)
        with pytest.raises(MaaError, match="cannot accumulate"):
            launch(ctx, c, presplit=pre)
        with pytest.raises(MaaError, match="GEGLU"):
            launch(ctx, R.Case(B=1, H=1, W=63, C1=64, Cout=128, geglu=True, res=True, seed=16), presplit=pre)
        g = R.Case(B=1, H=1, W=63, C1=64, Cout=128, geglu=True, seed=16)
        for extra in (dict(act=2), dict(out_scale=0.5), dict(accumulate=1)):
            with pytest.raises(MaaError, match="GEGLU"):
                launch(ctx, g, presplit=pre, **extra)
        n = R.Case(B=B, H=H, W=W, C1=R.CIN, Cout=78, bias=True, c2=True, seed=16)
        with pytest.raises(MaaError, match="32-channel lines" if pre else "only the fp32 engine"):
            launch(ctx, n, presplit=pre)
        if not pre:
            for terms in (dict(c_split=True), dict(c2=True)):
                with pytest.raises(MaaError, match="only the fp32 engine"):
                    launch(ctx, R.Case(B=B, H=H, W=W, C1=R.CIN, Cout=96, bias=True, seed=16, **terms))


# ------------------------------------------------------------------------------------------------ (d) GEGLU, fp32 and split32 output
def geglu_cases():
    for M in R.GEGLU_M:
        for packed in R.GEGLU_PACKED:
            for K in R.GEGLU_K:
                pad = R.LDC_PAD if M in (63, 257) else 0
                yield f"{M}x{K}x{packed}", R.case(B=1, H=1, W=M, C1=K, Cout=packed, geglu=True, ldc_pad=pad, seed=14)


def geglu_engine(engine, K):
    """(engine that runs, slices): one 32-channel chunk cannot be sliced, and the 1x1 ping-pong form needs two chunks."""
    if engine.startswith("PP1") and K < 64:
        return "DMA", None
    S = ENGINES[engine].get("S")
    return engine, (min(S, K // 32) if S else S)


@pytest.mark.parametrize("concurrency", [1, 3])
@pytest.mark.parametrize("precision", BF)
def test_geglu_split_output_on_the_dma_engine(ctxs, precision, concurrency):
    ctx = ctxs[precision]
    ctx.set_concurrency(concurrency)
    try:
        for name, c in geglu_cases():
            with forced("DMA"):
                y, _ = run(ctx, "DMA", c)
                ys, _ = run(ctx, "DMA", c, c_split=1)
            with forced("DMA_generic"):
                g, _ = run(ctx, "DMA_generic", c)
                gs, _ = run(ctx, "DMA_generic", c, c_split=1)
            check(f"igemm_geglu_DMA_{precision}_c{concurrency}_{name}", y, c.reference(precision)[0], R.GATE[precision])
            assert torch.equal(bits(y), bits(g)) and torch.equal(bits(ys), bits(gs)), name
            assert torch.equal(bits(ys), bits(split_of(y))), name
    finally:
        ctx.set_concurrency(None)


@pytest.mark.parametrize("engine", ["PP1_128_1", "PP1_128_2", "DMA2_s1", "DMA2_s2"])
@pytest.mark.parametrize("precision", BF)
def test_geglu_split_output_on_the_wide_tile_engines(ctxs, precision, engine):
    ctx = ctxs[precision]
    with forced(engine):
        for name, c in geglu_cases():
            runs, S = geglu_engine(engine, c.C1)
            y, _ = run(ctx, engine, c, slices=S, expect=runs)
            ys, _ = run(ctx, engine, c, slices=S, expect=runs, c_split=1)
            check(f"igemm_geglu_{engine}_{precision}_{name}", y, c.reference(precision)[0], R.GATE[precision])
            assert torch.equal(bits(ys), bits(split_of(y))), name


# ------------------------------------------------------------------------------------------------ (e) two sources
GATHERS = [("F32", "f32"), ("BF16_REG", "bf16x3"), ("BF16_REG", "bf16")]


@pytest.mark.parametrize("engine,precision", GATHERS)
def test_two_sources(ctxs, engine, precision):
    ctx = ctxs[precision]
    B, H, W = R.IMAGES[0]
    pairs = R.TWO_SOURCES + (R.TWO_SOURCES_UNALIGNED if engine == "F32" else ())
    with forced(engine):
        for C1, C2 in pairs:
            for k in R.KERNELS:
                c = R.case(B=B, H=H, W=W, C1=C1, C2=C2, ld1_pad=R.LD1_PAD, Cout=96, k=k, seed=15)
                y, _ = run(ctx, engine, c)
                check(f"igemm_two_{engine}_{precision}_{C1}+{C2}_k{k}", y, c.reference(precision)[0], R.GATE[precision])
                for tap in range(k * k):
                    p = R.Case(B=B, H=H, W=W, C1=C1, C2=C2, ld1_pad=R.LD1_PAD, Cout=C1 + C2, k=k, seed=15,
                               weight=R.one_hot_weight(C1 + C2, k, tap))
                    y, _ = run(ctx, engine, p)
                    ref = p.reference(precision)[0]
                    check(f"igemm_probe_{engine}_{precision}_{C1}+{C2}_k{k}_t{tap}", y, ref, R.GATE[precision])
                    if precision != "bf16x3":      # one product by 1.0 per output: exact (bf16x3 rebuilds x from hi + lo)
                        assert torch.equal(y.double(), ref), (C1, C2, k, tap)


@pytest.mark.parametrize("engine,precision", GATHERS)
def test_aligned_gather_over_read(ctxs, engine, precision):
    """K = 77 in rows of pitch 80: the last float4 of the aligned gather reads the three padding floats, which hold 30000 and must
    meet zero rows of B."""
    ctx = ctxs[precision]
    with forced(engine):
        for B, H, W in R.IMAGES:
            c = R.case(B=B, H=H, W=W, C1=77, ld1_pad=3, Cout=96, k=1, bias=True, seed=17)
            y, _ = run(ctx, engine, c)
            check(f"igemm_overread_{engine}_{precision}_b{B}", y, c.reference(precision)[0], R.GATE[precision])


@pytest.mark.parametrize("engine,precision", ON)
def test_a_side_leaky_and_virtual_upsample(ctxs, engine, precision):
    """The A-side terms of the descriptor beside an epilogue term: leaky-relu of A (applied while staging an fp32 A; with presplit
    it is in the packed rows, and the reference applies it in fp32 before any rounding), and the nearest-2x upsample read through
    the gather (3x3 only; the ping-pong engines do not take it and are left out)."""
    ctx = ctxs[precision]
    with forced(engine):
        for B, H, W in R.IMAGES:
            for k in kernels_of(engine):
                c = R.case(B=B, H=H, W=W, C1=R.CIN, Cout=96, k=k, bias=True, res=True, a_leaky=R.SLOPE, seed=18)
                y, _ = run(ctx, engine, c)
                check(f"igemm_aleaky_{engine}_{precision}_b{B}_k{k}", y, c.reference(precision)[0], R.GATE[precision])
                if k == 3 and not engine.startswith("PP"):
                    u = R.case(B=B, H=H, W=W, C1=R.CIN, Cout=78, k=3, bias=True, a_leaky=R.SLOPE, up=1, seed=19)
                    y, _ = run(ctx, engine, u)
                    check(f"igemm_up_{engine}_{precision}_b{B}", y, u.reference(precision)[0], R.GATE[precision])


# ------------------------------------------------------------------------------------------------ (g) contracts
def sample_of(c, b):
    """Sample b of a case as a case of its own: the same values, B = 1."""
    s = copy.copy(c)
    hw, mo = c.H * c.W, c.Ho * c.Wo
    s.B, s.M, s._ref = 1, mo, {}
    s.x1 = c.x1[b * hw * c.ld1:(b + 1) * hw * c.ld1].clone()
    s.x2 = c.x2[b * hw * c.ld2:(b + 1) * hw * c.ld2].clone() if c.x2 is not None else None
    s.rowadd = c.rowadd[b * c.ld_rowadd:].clone() if c.rowadd is not None else None
    s.res = c.res[b * mo * c.ldr:(b + 1) * mo * c.ldr].clone() if c.res is not None else None
    s.prior = c.prior[b * mo:(b + 1) * mo] if c.prior is not None else None
    s.c = R.out_buffer(mo, c.N, c.ldc, c.lead, s.prior)
    s.c2 = R.out_buffer(mo, c.N, c.ldc2, c.lead) if c.c2 is not None else None
    return s


def all_terms_cases(kernels):
    return list(R.term_cases(kernels=kernels, couts=(96, 77), names=("all_act3",)))


@pytest.mark.parametrize("engine,precision", ON)
def test_deterministic_and_batch_invariant_with_every_term(ctxs, engine, precision):
    ctx = ctxs[precision]
    with forced(engine):
        for name, c in all_terms_cases(kernels_of(engine)):
            y, _ = run(ctx, engine, c)
            again, _ = run(ctx, engine, c)
            assert torch.equal(bits(y), bits(again)), name
            b = c.B - 2
            mo = c.Ho * c.Wo
            alone, _ = run(ctx, engine, sample_of(c, b))
            assert torch.equal(bits(alone), bits(y[b * mo:(b + 1) * mo])), name


@pytest.mark.parametrize("precision", BF)
def test_engines_agree_bit_for_bit_with_every_term(ctxs, precision):
    """One product per k-step, k ascending, fp32 accumulation, one shared epilogue: without a K split the LDS-DMA engine, the second
    engine and the 1x1 ping-pong form return the register-staged engine's bits; two slices of the 1x1 form those of the second engine."""
    ctx = ctxs[precision]

    def on(engine, cases):
        with forced(engine):
            return [run(ctx, engine, c)[0] for _, c in cases]

    for k in R.KERNELS:
        cases = all_terms_cases((k,))
        reg = on("BF16_REG_split", cases)
        for engine in ("DMA", "DMA2_s1") + (("PP1_128_1",) if k == 1 else ()):
            for (name, _), y, r in zip(cases, on(engine, cases), reg):
                assert torch.equal(bits(y), bits(r)), (engine, name)
        if k == 1:
            for (name, _), y, r in zip(cases, on("PP1_128_2", cases), on("DMA2_s2", cases)):
                assert torch.equal(bits(y), bits(r)), name
