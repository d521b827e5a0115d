"""Test-side restatement of the contraction descriptor (IGemm, csrc/maa_internal.h) that tests/test_gpu_igemm_ops.py compares
maa_op_igemm_ex against: plain torch in float64, the same arguments on CPU tensors.

    A   = leaky(upsample2(x1 | x2), a_leaky)                         (the activation in fp32, as the kernels stage it)
    acc = conv2d(A, w)  with (pad_h, pad_w) zeros before, as many as needed after, cropped to Ho x Wo
    v   = act(alpha * acc + bias + rowadd[sample] + res) * out_scale  (+ c with accumulate)
    geglu: v = value * gelu(gate) of (alpha * acc + bias), value = rows [0, inner) of w, gate = rows [inner, 2 inner)
    c2  = leaky(v, c2_slope)

In the plain-bf16 mode the kernels multiply the operands rounded to bf16, so the reference rounds A (after its activation) and
the weights there too, as tests/test_gpu_linear_variants.py does; what is left in every mode is the summation order.

Also here: the padded buffers of the GPU cases (inputs with a large finite fill in their pitch padding, outputs with one bit
pattern everywhere), the case tables, and the deliberate mistakes tests/test_igemm_ref.py shows to be visible at the gates.
The split32 codec is tests/attn_ref.py's (one copy for the operator files that need it)."""
import math

import torch
import torch.nn.functional as F

from tests.attn_ref import gen, rel_max, split32_decode, split32_encode      # noqa: F401  (shared with the GPU file)

GATE = {"f32": 2e-5, "bf16x3": 2e-4, "bf16": 2e-5}      # tests/test_gpu_ops.py, tests/test_gpu_pp.py, tests/test_gpu_linear_variants.py
SLOPE = 0.1
FILL_IN = 30000.0                 # pitch padding of the inputs: large, finite (gather_aligned's over-read must meet finite values)
FILL_OUT = 0x7F4A7C15             # every float of an output buffer before the launch (2.69e38 as fp32: finite, never a result)

MISTAKES = ("scale_before_act", "act_before_res", "rowadd_next_sample", "rowadd_pitch_n", "sources_swapped", "c2_pre_act",
            "geglu_halves")


def rows_of(buf, rows, ld, C):
    """The [rows, C] matrix that starts at the first float of `buf` with row pitch ld."""
    flat = buf.reshape(-1)
    assert flat.numel() >= (rows - 1) * ld + C, (flat.numel(), rows, ld, C)
    return flat.as_strided((rows, C), (ld, 1))


def leaky32(x, slope):
    """leaky-relu in fp32, one rounded multiplication: what the kernels apply to an fp32 operand."""
    x = x.to(torch.float32)
    return torch.where(x > 0, x, x * torch.tensor(slope, dtype=torch.float32))


def operand(t, precision):
    """What the mode multiplies, as float64: the fp32 value, or in plain bf16 its rounding to bf16."""
    t = t.to(torch.float32)
    return (t.to(torch.bfloat16) if precision == "bf16" else t).to(torch.float64)


def activation(v, act, slope):
    if act == 1:
        return torch.tanh(v)
    if act == 2:
        return v.clamp_min(0.0)
    if act == 3:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == 4:
        return torch.where(v > 0, v, v * slope)
    assert act == 0
    return v


def igemm_ref(x1, ld1, C1, x2, ld2, C2, B, H, W, Ho, Wo, w, bias, c, ldc, stride=1, pad_w=0, pad_h=-1, dil=1, up=0, a_leaky=0.0,
              presplit=0, alpha=1.0, rowadd=None, ld_rowadd=0, res=None, ldr=0, act=0, act_slope=0.0, out_scale=1.0, accumulate=0,
              geglu=0, c_split=0, c2=None, ldc2=0, c2_slope=1.0, precision="f32", mistake=None, dtype=torch.float64):
    """The arguments of Context.op_igemm_ex on CPU tensors (`c` is read only with accumulate; presplit, c_split, ldc2 change the
    form of what is stored, not its value).  Returns (c, c2) as [B Ho Wo, N] in `dtype`, c2 None without a second output.
    mistake: one of MISTAKES.  dtype = torch.float32 gives the fp32 torch restatement of the same case."""
    assert mistake is None or mistake in MISTAKES
    M = B * Ho * Wo
    w = w.detach().to("cpu", torch.float32)
    if w.dim() == 2:
        w = w[:, :, None, None]
    Cout, Ctot, KH, KW = w.shape
    assert Ctot == C1 + C2
    srcs = [rows_of(x1, B * H * W, ld1, C1)]
    if C2:
        srcs.append(rows_of(x2, B * H * W, ld2, C2))
    if mistake == "sources_swapped":
        srcs.reverse()
    a = torch.cat(srcs, dim=1).reshape(B, H, W, Ctot).permute(0, 3, 1, 2)
    if up:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    if a_leaky != 0.0:
        a = leaky32(a, a_leaky)
    if dtype == torch.float64:
        a, wk = operand(a, precision), operand(w, precision)
    else:
        a, wk = a.to(dtype), w.to(dtype)
    ph = pad_h if pad_h >= 0 else (pad_w if KH > 1 else 0)
    He, We = a.shape[2], a.shape[3]
    after_h = max(0, (Ho - 1) * stride + dil * (KH - 1) + 1 - (He + ph))
    after_w = max(0, (Wo - 1) * stride + dil * (KW - 1) + 1 - (We + pad_w))
    acc = F.conv2d(F.pad(a, (pad_w, after_w, ph, after_h)), wk, None, stride=stride, dilation=dil)[:, :, :Ho, :Wo]
    acc = acc.permute(0, 2, 3, 1).reshape(M, Cout)
    v = acc * alpha
    if bias is not None:
        v = v + bias.detach().to("cpu", dtype)
    if geglu:
        val, gate = v.chunk(2, dim=1)
        if mistake == "geglu_halves":
            val, gate = gate, val
        return val * activation(gate, 3, 0.0), None
    N = Cout
    if rowadd is not None:
        pitch = N if mistake == "rowadd_pitch_n" else ld_rowadd
        ra = rows_of(rowadd, B, pitch, N).to(dtype)
        if mistake == "rowadd_next_sample":
            ra = ra.roll(-1, dims=0)
        v = (v.reshape(B, Ho * Wo, N) + ra[:, None, :]).reshape(M, N)
    r = rows_of(res, M, ldr, N).to(dtype) if res is not None else 0.0
    if mistake == "act_before_res":
        pre = v
        v = activation(v, act, act_slope) + r
    else:
        pre = v + r
        v = activation((pre * out_scale) if mistake == "scale_before_act" else pre, act, act_slope)
    if mistake != "scale_before_act":
        v = v * out_scale
    if accumulate:
        v = v + rows_of(c, M, ldc, N).to(dtype)
    y2 = None
    if c2 is not None:
        s = pre if mistake == "c2_pre_act" else v
        y2 = torch.where(s > 0, s, s * c2_slope)
    return v, y2


# ------------------------------------------------------------------------------------------------ buffers
def padded_in(x, ld, lead=0):
    """[rows, C] -> a flat buffer of lead + rows * ld floats holding x with row pitch ld from float `lead`; FILL_IN elsewhere."""
    rows, C = x.shape
    assert ld >= C
    buf = torch.full((lead + rows * ld,), FILL_IN, dtype=torch.float32)
    rows_of(buf[lead:], rows, ld, C).copy_(x)
    return buf


SPARE_ROWS = 3


def out_buffer(M, N, ld, lead=0, prior=None):
    """A flat output buffer of lead + (M + SPARE_ROWS) * ld floats, every float FILL_OUT; prior [M, N] (the accumulate target) is
    laid into the result's place."""
    buf = torch.full((lead + (M + SPARE_ROWS) * ld,), FILL_OUT, dtype=torch.int32).view(torch.float32)
    if prior is not None:
        rows_of(buf[lead:], M, ld, N).copy_(prior)
    return buf


def outside_untouched(buf, M, N, ld, lead=0):
    """True when every float of an out_buffer outside [M rows] x [N columns] still holds FILL_OUT, bit for bit."""
    bits = buf.detach().to("cpu").reshape(-1).view(torch.int32).clone()
    rows_of(bits[lead:], M, ld, N).fill_(FILL_OUT)
    return bool((bits == FILL_OUT).all())


# ------------------------------------------------------------------------------------------------ cases
IMAGES = ((3, 5, 7), (5, 3, 5))      # B, H, W: 35 rows per sample (32-row blocks straddle samples at 35 and 70) / 15 (RSEL false)
CIN = 64                             # 18 chunks for a 3x3, two for a 1x1: enough for two K slices
COUTS = (96, 78, 77)                 # split32-capable and ragged against 64 / 128 / 160; even with a ragged 32-column block; odd
KERNELS = (3, 1)
ROWADD_OFF = 32                      # the row add is columns 32 .. 32 + N of a [B, N + 32] slab
RES_PAD = 8                          # ldr = N + 8
LDC_PAD = 8                          # ldc = N + 8

# group (a): one term at a time, then all at once with each activation in turn
TERMS = {
    "plain": dict(),
    "alpha": dict(alpha=0.5),
    "bias": dict(bias=True),
    "rowadd": dict(rowadd=True),
    "res": dict(res=True),
    "tanh": dict(act=1),
    "relu": dict(act=2),
    "gelu": dict(act=3),
    "leaky": dict(act=4),
    "out_scale": dict(out_scale=1.0 / 3.0),
    "accumulate": dict(accumulate=True),
    "ldc": dict(ldc_pad=LDC_PAD),
}
ALL_TERMS = dict(alpha=0.5, bias=True, rowadd=True, res=True, out_scale=1.0 / 3.0, accumulate=True, ldc_pad=LDC_PAD)
for _a in range(5):
    TERMS["all_act%d" % _a] = dict(ALL_TERMS, act=_a)

# group (b): store-form selection -- (Cout, ldc pad, lead floats, c2)
STORE_FORMS = ((78, 0, 0, False), (78, 2, 0, False), (78, 1, 0, False), (78, 0, 1, False), (78, 2, 1, False), (77, 0, 0, False),
               (77, 1, 0, False), (96, 0, 0, False), (96, 0, 0, True), (96, 1, 0, True), (96, 0, 1, True), (96, 0, 1, False))

# group (c): split32 outputs on the 96-wide cases
SPLIT_OUTS = {
    "split_bias_res": dict(bias=True, res=True, c_split=True),
    "split_gelu": dict(bias=True, act=3, c_split=True),
    "split_rowadd": dict(rowadd=True, c_split=True),
    "c2_leaky": dict(bias=True, act=4, c2=True),
}

# group (d): GEGLU -- the M / packed N / K tables of tests/test_gpu_linear_variants.py
GEGLU_M = (1, 63, 130, 257)
GEGLU_PACKED = (128, 320)
GEGLU_K = (32, 320)

# group (e): two sources
TWO_SOURCES = ((64, 32), (32, 96))
TWO_SOURCES_UNALIGNED = ((9, 4), (20, 12))      # the exact-fp32 engine's per-element gather
LD1_PAD = 32


class Case:
    """One call: CPU buffers, the keyword arguments of op_igemm_ex / igemm_ref that go with them, and where the result lies."""

    def __init__(self, B, H, W, C1, Cout, k=1, C2=0, ld1_pad=0, bias=False, rowadd=False, res=False, act=0, alpha=1.0,
                 out_scale=1.0, accumulate=False, ldc_pad=0, lead=0, c_split=False, c2=False, geglu=False, a_leaky=0.0, up=0,
                 weight=None, seed=0):
        self.B, self.H, self.W, self.C1, self.C2 = B, H, W, C1, C2
        self.Ho, self.Wo = (2 * H, 2 * W) if up else (H, W)
        self.M = B * self.Ho * self.Wo
        self.N = N = Cout // 2 if geglu else Cout
        rows, Ctot = B * H * W, C1 + C2
        g = lambda i: gen(1000 * seed + i)
        self.ld1, self.ld2 = C1 + ld1_pad, C2
        self.x1 = padded_in(torch.randn(rows, C1, generator=g(1)), self.ld1)
        self.x2 = padded_in(torch.randn(rows, C2, generator=g(2)), self.ld2) if C2 else None
        if weight is None:
            weight = torch.randn(Cout, Ctot, k, k, generator=g(3)) / math.sqrt(k * k * Ctot)
            if geglu:
                weight = weight[:, :, 0, 0].contiguous()
        self.w = weight
        self.bias = torch.randn(Cout, generator=g(4)) if (bias or geglu) else None
        self.ld_rowadd = N + ROWADD_OFF
        slab = torch.randn(B * self.ld_rowadd, generator=g(5))      # a wide product: every column of the slab holds a value
        self.rowadd = slab[ROWADD_OFF:] if rowadd else None
        self.ldr = N + RES_PAD
        self.res = padded_in(torch.randn(self.M, N, generator=g(6)), self.ldr) if res else None
        self.ldc, self.lead = N + ldc_pad, lead
        self.prior = torch.randn(self.M, N, generator=g(7)) if accumulate else None
        self.c = out_buffer(self.M, N, self.ldc, lead, self.prior)
        self.ldc2 = N + ldc_pad
        self.c2 = out_buffer(self.M, N, self.ldc2, lead) if c2 else None
        self.kw = dict(stride=1, pad_w=k // 2, pad_h=-1, dil=1, up=int(up), a_leaky=a_leaky, alpha=alpha, act=act, act_slope=SLOPE,
                       out_scale=out_scale, accumulate=int(accumulate), geglu=int(geglu), c_split=int(c_split), c2_slope=SLOPE)
        self._ref = {}

    def call(self, fn, x1, x2, rowadd, res, c, c2, **extra):
        """fn = Context.op_igemm_ex or igemm_ref, on this case's buffers (or their device copies)."""
        kw = dict(self.kw, rowadd=rowadd, ld_rowadd=self.ld_rowadd if rowadd is not None else 0, res=res,
                  ldr=self.ldr if res is not None else 0, c2=c2, ldc2=self.ldc2 if c2 is not None else 0)
        kw.update(extra)
        return fn(x1, self.ld1, self.C1, x2, self.ld2, self.C2, self.B, self.H, self.W, self.Ho, self.Wo, self.w, self.bias, c,
                  self.ldc, **kw)

    def reference(self, precision, mistake=None, dtype=torch.float64):
        """(c, c2) of igemm_ref, computed once per (precision, mistake, dtype) and shared by every engine that runs the case."""
        key = (precision if dtype == torch.float64 else "f32", mistake, dtype)
        if key not in self._ref:
            self._ref[key] = self.call(igemm_ref, self.x1, self.x2, self.rowadd, self.res, self.c[self.lead:],
                                       self.c2[self.lead:] if self.c2 is not None else None, precision=precision,
                                       mistake=mistake, dtype=dtype)
        return self._ref[key]


_cases = {}


def case(**spec):
    """Case(**spec), built once per spec (the GPU tests of every engine and the CPU test share the inputs and the reference)."""
    key = tuple(sorted((k, v if not torch.is_tensor(v) else id(v)) for k, v in spec.items()))
    if key not in _cases:
        _cases[key] = Case(**spec)
    return _cases[key]


def term_cases(kernels=KERNELS, couts=COUTS, names=None):
    """Group (a): (name, Case) over images x kernel sizes x widths x term sets."""
    for B, H, W in IMAGES:
        for k in kernels:
            for Cout in couts:
                for name, terms in TERMS.items():
                    if names is None or name in names:
                        yield "%s_b%d_%dx%d_k%d_n%d" % (name, B, H, W, k, Cout), case(B=B, H=H, W=W, C1=CIN, Cout=Cout, k=k, seed=11, **terms)


def one_hot_weight(Ctot, k, tap):
    """Output channel n copies concatenated channel n of one tap."""
    w = torch.zeros(Ctot, Ctot, k, k)
    w[torch.arange(Ctot), torch.arange(Ctot), tap // k, tap % k] = 1.0
    return w
