"""Handle objects over the C ABI: context, UNet, VAE, vocoder, and the single-operator entry points.

torch is used for device buffers and the stream only; every computation below happens inside
libaudiogpt_mi355x.so.  All tensors at this boundary are fp32, contiguous, in the reference's layouts.
"""
import ctypes as C
import threading
import weakref

import numpy as np
import torch

from . import _lib as L


def default_precision():
    """Precision mode of the drop-in tool / sampler / vocoder classes when none is given: bf16x3 (meets the fp32
    parity gates), overridable with AUDIOGPT_AMD_PRECISION=f32|bf16x3|bf16."""
    import os
    p = os.environ.get("AUDIOGPT_AMD_PRECISION", "bf16x3")
    if p not in Context.PRECISIONS:
        raise ValueError("AUDIOGPT_AMD_PRECISION must be one of %s" % sorted(Context.PRECISIONS))
    return p


_contexts = weakref.WeakSet()


def reload_tuning():
    """Make every live context parse the MAA_* tuning environment again (it is read when a context is created): tests and
    A/B scripts call this after changing os.environ."""
    for c in list(_contexts):
        c.reload_tuning()


def _f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class _Handle:
    """What every object over a library handle repeats: `h` made by a create entry on a context, calls that pass (context, handle)
    first under the context's lock, output tensors on the context's device, and close / __del__ through the destroy entry the
    class names.  A new model handle sets `_destroy`, calls `_create` in its __init__ and `_call` in its methods."""

    _destroy = None          # the name of the maa_*_destroy entry

    def _create(self, ctx, entry, *args, state_dict=None):
        """self.h = what the create entry `entry` makes on `ctx` from `args` (then, with a state_dict, its tensor list)."""
        self.ctx, self.lib, self.device = ctx, ctx.lib, ctx.device
        if state_dict is not None:
            arr, n, keep = L.tensor_list(state_dict)      # `keep`: the host copies `arr` points into live until the call is over
            args += (arr, n)
        h = C.c_void_p()
        ctx._call(entry, *args, C.byref(h))
        self.h = h

    def _call(self, entry, *args):
        """entry(context, this handle, *args) under the context's lock; raises MaaError on a non-zero status."""
        self.ctx._call(entry, self.h, *args)

    def _empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One (device, stream) execution context.  Calls are serialised with a lock, like the reference's
    non re-entrant sampler (ddim.py:27-56)."""

    PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2}
    _destroy = "maa_ctx_destroy"

    def __init__(self, device="cuda:0", stream=None, precision="f32"):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.MaaError("no MI355X visible: the HIP backend has no CPU fallback")
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        torch.cuda.set_device(idx)
        # stream=None: the library creates its own (blocking) HIP stream, which orders against PyTorch's
        # default stream and can be captured into a hipGraph; pass a torch.cuda.Stream to share one.
        self._stream = stream
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
        h = C.c_void_p()
        L.check(self.lib.maa_ctx_create(idx, sp, C.byref(h)))
        self.h = h
        self.lock = threading.RLock()
        self.precision = "f32"
        self.set_precision(precision)
        _contexts.add(self)

    def _call(self, entry, *args):
        """entry(this context, *args) under the lock; raises MaaError on a non-zero status."""
        with self.lock:
            L.check(getattr(self.lib, entry)(self.h, *args))

    def reload_tuning(self):
        if getattr(self, "h", None):
            self._call("maa_ctx_reload_tuning")

    def set_precision(self, precision):
        """Arithmetic of the contractions for models created from now on (and for the op_* calls)."""
        self._call("maa_ctx_set_precision", self.PRECISIONS[precision])
        self.precision = precision

    def set_cfg_split(self, mode):
        """Classifier-free guidance inside `ddim_sample`: True -> the two halves of the UNet batch as two lanes (two branches of
        the captured step graph), False -> one stream, None -> the default policy: two lanes unless the context has been told that three or more are in
        flight on the device (`set_concurrency`; one batch owning the GPU gains 4 %, with three in flight the extra lanes lose up to 24 %).  The results are the same bit for bit."""
        self._call("maa_ctx_set_cfg_split", -1 if mode is None else int(bool(mode)))

    def set_concurrency(self, n):
        """The serving arrangement as a hint: how many contexts' launches the caller keeps in flight on this device (None: not told,
        treated as 1).  >= 3: one stream per guided DDIM step and tiles by least total workgroup time; 1 or 2: this
        context (nearly) owns the GPU (two CFG lanes, tiles by least launch time).  Bit-identical either way (include/maa.h)."""
        self._call("maa_ctx_set_concurrency", -1 if n is None else int(n))

    def synchronize(self):
        self._call("maa_ctx_synchronize")

    def workspace_bytes(self):
        n = C.c_size_t()
        self._call("maa_ctx_workspace_bytes", C.byref(n))
        return n.value

    def prof_begin(self, detail=False):
        """Start per-kernel hipEvent timing of every launch on this context (eager launches only)."""
        self._call("maa_prof_begin", int(detail))

    def prof_end(self):
        """Stop timing; returns {kernel: dict(launches, ms, flops, bytes)}."""
        rows = (L.maa_prof_row * 512)()
        n = C.c_int()
        self._call("maa_prof_end", rows, 512, C.byref(n))
        return {rows[i].name.decode(): dict(launches=int(rows[i].launches), ms=rows[i].ms, flops=rows[i].flops,
                                            bytes=rows[i].bytes) for i in range(n.value)}

    def calib(self):
        """Box calibration (csrc/calib.hip): what a fixed MFMA loop, a fixed device copy and fixed re-reads out of L2 / out of
        the Infinity Cache reach on this box right now."""
        out = {}
        for kind, key in ((0, "mfma_bf16_tflops"), (1, "copy_gbs"), (2, "l2_read_gbs"), (3, "infinity_cache_read_gbs")):
            v = C.c_double()
            self._call("maa_calib", kind, C.byref(v))
            out[key] = v.value
        return out

    # ---- single operators (parity tests / kernel profiling) -------------------------------------
    def op_linear(self, a, w, b=None, geglu=False, res=None, split_out=False):
        """a [M,K]; w [N,K]; res [M,N] is added to the result.  split_out: the [M,N] floats returned hold split32 rows (per 32 columns
        32 bf16 hi, then 32 bf16 lo)."""
        a = _f32(a, self.device)
        M, K = a.shape
        N = w.shape[0]
        wt, wp = L.host_f32(w)
        bt, bp = L.host_f32(b) if b is not None else (None, None)
        y = self._empty(M, N // 2 if geglu else N)
        r = _f32(res, self.device) if res is not None else None
        assert r is None or tuple(r.shape) == tuple(y.shape)
        self._call("maa_op_linear", L.dptr(a), M, K, wp, bp, N, int(geglu), L.dptr(y), L.dptr(r) if r is not None else None,
                   int(split_out))
        return y

    def op_conv(self, x, w, b=None, stride=1, pad=0, dil=1, up=False, leaky=0.0, out_hw=None, rowadd=None, res=None,
                split_out=False):
        """x [B,Cin,H,W]; w [Cout,Cin,KH,KW]; returns [B,Cout,Ho,Wo].  rowadd [B,Cout] and res [B,Cout,Ho,Wo] are added to the
        result.  split_out: returns the channels-last result [B,Ho,Wo,Cout] as split32 rows instead (see op_linear), as the
        convolutions that feed a contraction write it."""
        x = _f32(x, self.device)
        B, Cin, H, W = x.shape
        Cout, _, KH, KW = w.shape
        if out_hw is None:
            He, We = (2 * H, 2 * W) if up else (H, W)
            ph = pad if KH > 1 else 0
            Ho = (He + 2 * ph - dil * (KH - 1) - 1) // stride + 1
            Wo = (We + 2 * pad - dil * (KW - 1) - 1) // stride + 1
        else:
            Ho, Wo = out_hw
        wt, wp = L.host_f32(w)
        bt, bp = L.host_f32(b) if b is not None else (None, None)
        y = self._empty((B, Ho, Wo, Cout) if split_out else (B, Cout, Ho, Wo))
        ra = _f32(rowadd, self.device) if rowadd is not None else None
        r = _f32(res, self.device) if res is not None else None
        assert ra is None or tuple(ra.shape) == (B, Cout)
        assert r is None or tuple(r.shape) == (B, Cout, Ho, Wo)
        self._call("maa_op_conv", L.dptr(x), B, Cin, H, W, wp, bp, Cout, KH, KW, stride, pad, dil, int(up), float(leaky), L.dptr(y),
                   Ho, Wo, L.dptr(ra) if ra is not None else None, L.dptr(r) if r is not None else None, int(split_out))
        return y

    def op_groupnorm(self, x, gamma, beta, eps, silu=False):
        x = _f32(x, self.device)
        B, Cc = x.shape[:2]
        HW = int(np.prod(x.shape[2:]))
        gt, gp = L.host_f32(gamma)
        bt, bp = L.host_f32(beta)
        y = torch.empty_like(x)
        self._call("maa_op_groupnorm", L.dptr(x), B, Cc, HW, gp, bp, float(eps), int(silu), L.dptr(y))
        return y

    def op_layernorm(self, x, gamma, beta, eps=1e-5):
        x = _f32(x, self.device)
        rows, Cc = x.reshape(-1, x.shape[-1]).shape
        gt, gp = L.host_f32(gamma)
        bt, bp = L.host_f32(beta)
        y = torch.empty_like(x)
        self._call("maa_op_layernorm", L.dptr(x), rows, Cc, gp, bp, float(eps), L.dptr(y))
        return y

    def op_attention(self, q, k, v, heads, alpha):
        q, k, v = _f32(q, self.device), _f32(k, self.device), _f32(v, self.device)
        B, Nq, Cc = q.shape
        Nk = k.shape[1]
        y = torch.empty_like(q)
        self._call("maa_op_attention", L.dptr(q), L.dptr(k), L.dptr(v), B, heads, Cc // heads, Nq, Nk, float(alpha), L.dptr(y))
        return y

    def op_attention_ex(self, q, ldq, hsq, k, ldk, hsk, v, ldv, hsv, B, heads, dh, Nq, Nk, alpha, out, ldo,
                        out_split=0, causal=0):
        """maa_op_attention_ex: the library's internal attention call on device tensors the caller has laid out
        (q / k / v / out are fp32 device tensors, possibly views into one buffer; pitches and head strides in floats).
        Writes into `out`; nothing is allocated, copied or checked beyond what the C entry point checks."""
        for t in (q, k, v, out):
            assert t.is_cuda and t.dtype == torch.float32, (t.device, t.dtype)
        self._call("maa_op_attention_ex", C.c_void_p(q.data_ptr()), int(ldq), int(hsq), C.c_void_p(k.data_ptr()), int(ldk),
                   int(hsk), C.c_void_p(v.data_ptr()), int(ldv), int(hsv), int(B), int(heads), int(dh), int(Nq), int(Nk),
                   float(alpha), C.c_void_p(out.data_ptr()), int(ldo), int(out_split), int(causal))
        return out

    def op_attention_masked(self, q, ldq, hsq, k, ldk, hsk, v, ldv, hsv, B, heads, dh, Nq, Nk, alpha, out, ldo, key_mask,
                            out_split=0, causal=0):
        """maa_op_attention_masked: op_attention_ex with MultiheadAttention's key_padding_mask, key_mask [B, Nk] fp32 on the
        device, non-zero = hidden from every query of its sample."""
        for t in (q, k, v, out, key_mask):
            assert t.is_cuda and t.dtype == torch.float32, (t.device, t.dtype)
        assert key_mask.is_contiguous() and tuple(key_mask.shape) == (B, Nk), tuple(key_mask.shape)
        self._call("maa_op_attention_masked", C.c_void_p(q.data_ptr()), int(ldq), int(hsq), C.c_void_p(k.data_ptr()), int(ldk),
                   int(hsk), C.c_void_p(v.data_ptr()), int(ldv), int(hsv), int(B), int(heads), int(dh), int(Nq), int(Nk),
                   float(alpha), C.c_void_p(out.data_ptr()), int(ldo), int(out_split), int(causal), C.c_void_p(key_mask.data_ptr()))
        return out

    def op_groupnorm_ex(self, x1, ld1, C1, x2, ld2, C2, B, HW, groups, gamma, beta, eps, silu, out, out_split=0, raw=None):
        """maa_op_groupnorm_ex: the library's internal GroupNorm call on channels-last device tensors the caller has laid out
        (x1 / x2 / out / raw are fp32 device tensors, possibly views into wider buffers; pitches in floats; x2 None with C2 = 0 for
        one source).  Writes into `out` (and `raw`); nothing is allocated, copied or checked beyond what the C entry point checks."""
        for t in (x1, x2, out, raw):
            assert t is None or (t.is_cuda and t.dtype == torch.float32), (t.device, t.dtype)
        gt, gp = L.host_f32(gamma)
        bt, bp = L.host_f32(beta)
        assert gt.numel() == C1 + C2 and bt.numel() == C1 + C2
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._call("maa_op_groupnorm_ex", ptr(x1), int(ld1), int(C1), ptr(x2), int(ld2), int(C2), int(B), int(HW), int(groups), gp,
                   bp, float(eps), int(silu), ptr(out), int(out_split), ptr(raw))
        return out

    def op_igemm_ex(self, x1, ld1, C1, x2, ld2, C2, B, H, W, Ho, Wo, w, bias, c, ldc, stride=1, pad_w=0, pad_h=-1, dil=1, up=0,
                    a_leaky=0.0, presplit=0, alpha=1.0, rowadd=None, ld_rowadd=0, res=None, ldr=0, act=0, act_slope=0.0,
                    out_scale=1.0, accumulate=0, geglu=0, c_split=0, c2=None, ldc2=0, c2_slope=1.0):
        """maa_op_igemm_ex: the library's internal contraction call (conv_into -> launch_igemm) with every field of its descriptor, on
        channels-last device tensors the caller has laid out (x1 / x2 / rowadd / res / c / c2 are fp32 device tensors, possibly views
        into wider buffers; pitches in floats; x2 None with C2 = 0 for one source).  w [Cout, C1+C2, KH, KW] (geglu: [2 inner, K]) and
        bias come from the host.  Writes into `c` (and `c2`); nothing is allocated, copied or checked beyond what the C entry point
        checks."""
        for t in (x1, x2, rowadd, res, c, c2):
            assert t is None or (t.is_cuda and t.dtype == torch.float32), (t.device, t.dtype)
        wt, wp = L.host_f32(w)
        bt, bp = L.host_f32(bias) if bias is not None else (None, None)
        ptr = lambda t: t.data_ptr() if t is not None else None
        KH, KW = (1, 1) if wt.dim() == 2 else (int(wt.shape[2]), int(wt.shape[3]))
        assert wt.shape[1] == C1 + C2 and (bt is None or bt.numel() == wt.shape[0])
        a = L.maa_igemm_ex_args(
            d_x1=ptr(x1), ld1=int(ld1), C1=int(C1), d_x2=ptr(x2), ld2=int(ld2), C2=int(C2), B=int(B), H=int(H), W=int(W), Ho=int(Ho),
            Wo=int(Wo), h_w=wp, h_bias=bp, Cout=int(wt.shape[0]), KH=KH, KW=KW, stride=int(stride), pad_w=int(pad_w), pad_h=int(pad_h),
            dil=int(dil), up=int(up), a_leaky=float(a_leaky), presplit=int(presplit), alpha=float(alpha), d_rowadd=ptr(rowadd),
            ld_rowadd=int(ld_rowadd), d_res=ptr(res), ldr=int(ldr), act=int(act), act_slope=float(act_slope),
            out_scale=float(out_scale), accumulate=int(accumulate), geglu=int(geglu), c_split=int(c_split), d_c=ptr(c), ldc=int(ldc),
            d_c2=ptr(c2), ldc2=int(ldc2), c2_slope=float(c2_slope))
        self._call("maa_op_igemm_ex", C.byref(a))
        return c

    def op_seq_rows(self, kind, x, out, C_, rows=0, B=0, T=0, res=None, mask=None, scale=None, shift=None, gamma=None, beta=None,
                    w=None, bias=None, groups=0, eps=1e-5, table_rows=0, alpha=1.0, n_out=0, pitch_norm=0, f0_mean=0.0, f0_std=1.0,
                    use_uv=0, out2=None, pos=None, dur=None):
        """maa_op_seq_rows: one row operator of the sequence models through the library's internal launch (`kind`: a key of
        _lib.SEQ_KINDS; include/maa.h lists what each reads and writes).  x / res / mask / out / out2 are fp32 device tensors and
        pos / dur int32 ones, possibly views into larger buffers (out may be x where the header allows it); scale / shift / gamma /
        beta / w / bias come from the host.  Writes into the outputs; nothing is allocated, copied or checked beyond what the C
        entry point checks."""
        for t in (x, res, mask, out, out2):
            assert t is None or (t.is_cuda and t.dtype == torch.float32), (t.device, t.dtype)
        for t in (pos, dur):
            assert t is None or (t.is_cuda and t.dtype == torch.int32), (t.device, t.dtype)
        keep = [L.host_f32(t) if t is not None else (None, None) for t in (scale, shift, gamma, beta, w, bias)]
        ptr = lambda t: t.data_ptr() if t is not None else None
        a = L.maa_seq_rows_args(
            kind=L.SEQ_KINDS[kind], rows=int(rows), B=int(B), T=int(T), C=int(C_), d_x=ptr(x), d_res=ptr(res), d_mask=ptr(mask),
            h_scale=keep[0][1], h_shift=keep[1][1], h_gamma=keep[2][1], h_beta=keep[3][1], h_w=keep[4][1], h_bias=keep[5][1],
            groups=int(groups), eps=float(eps), table_rows=int(table_rows), alpha=float(alpha), n_out=int(n_out),
            pitch_norm=int(pitch_norm), f0_mean=float(f0_mean), f0_std=float(f0_std), use_uv=int(use_uv), d_out=ptr(out),
            d_out2=ptr(out2), d_pos=ptr(pos), d_dur=ptr(dur))
        self._call("maa_op_seq_rows", C.byref(a))
        return out

    def op_tts_rows(self, kind, **fields):
        """maa_op_tts_rows: one row kernel of the Glow post-net or of the plain FastSpeech2 through the library's internal launch
        (`kind`: a key of _lib.TTS_KINDS; include/maa.h lists what each reads and writes).  `fields` are the members of
        maa_tts_rows_args by name: integers and floats as they are, d_* as device tensors (fp32; int32 for d_tok / d_mel2ph / d_ids /
        d_bin), possibly views into larger buffers, h_* as host tensors.  Nothing is allocated, copied or checked beyond what the C
        entry point checks."""
        a = L.maa_tts_rows_args(kind=L.TTS_KINDS[kind])
        types = dict(L.maa_tts_rows_args._fields_)
        keep = []
        for name, v in fields.items():
            assert name in types and name != "kind", name
            if v is None:
                continue
            if name.startswith("h_"):
                keep.append(L.host_f32(v))
                v = keep[-1][1]
            elif name.startswith("d_"):
                assert v.is_cuda and v.dtype == (torch.int32 if name in ("d_tok", "d_mel2ph", "d_ids", "d_bin") else torch.float32), \
                    (name, v.device, v.dtype)
                v = v.data_ptr()
            else:
                v = float(v) if types[name] is C.c_float else int(v)
            setattr(a, name, v)
        self._call("maa_op_tts_rows", C.byref(a))

    def op_sampler_step(self, kind, **fields):
        """maa_op_sampler_step: one step kernel of the sampling loops through the library's internal launch (`kind`: a key of
        _lib.STEP_KINDS; include/maa.h lists what each reads and writes).  `fields` are the members of maa_sampler_step_args by
        name: integers and floats as they are, d_* as device tensors (fp32, or int32 for d_step / d_st), possibly views into larger
        buffers, or raw addresses.  Nothing is allocated, copied or checked beyond what the C entry point checks."""
        a = L.maa_sampler_step_args(kind=L.STEP_KINDS[kind])
        known = {f[0] for f in L.maa_sampler_step_args._fields_}
        for name, v in fields.items():
            assert name in known, name
            if torch.is_tensor(v):
                assert v.is_cuda and v.dtype == (torch.int32 if name in ("d_step", "d_st") else torch.float32), (name, v.device, v.dtype)
                v = v.data_ptr()
            setattr(a, name, v)
        self._call("maa_op_sampler_step", C.byref(a))

    def op_front_rows(self, kind, x, out, scale=None, shift=None, **fields):
        """maa_op_front_rows: one small kernel of the waveform front ends / of Cnn14's ends through the library's internal launch
        (`kind`: a key of _lib.FRONT_KINDS; include/maa.h lists what each reads and writes).  x / out are fp32 device tensors,
        possibly views into larger buffers; scale / shift ("affine") come from the host; `fields` are the integer and float
        members of maa_front_rows_args by name.  Writes into `out`; nothing is allocated, copied or checked beyond what the C
        entry point checks."""
        for t in (x, out):
            assert t.is_cuda and t.dtype == torch.float32, (t.device, t.dtype)
        keep = [L.host_f32(t) if t is not None else (None, None) for t in (scale, shift)]
        a = L.maa_front_rows_args(kind=L.FRONT_KINDS[kind], d_x=x.data_ptr(), d_out=out.data_ptr(), h_scale=keep[0][1],
                                  h_shift=keep[1][1])
        known = {f[0]: f[1] for f in L.maa_front_rows_args._fields_ if f[1] in (C.c_int, C.c_float)}
        for name, v in fields.items():
            assert name in known and name != "kind", name
            setattr(a, name, float(v) if known[name] is C.c_float else int(v))
        self._call("maa_op_front_rows", C.byref(a))
        return out

    def op_layernorm_ex(self, x, gamma, beta, eps=1e-5, out_split=0):
        """LayerNorm over the last dim of x [rows, C]; out_split = 1: the result as split32 rows in an fp32-typed tensor."""
        x = _f32(x, self.device)
        rows, Cc = x.reshape(-1, x.shape[-1]).shape
        gt, gp = L.host_f32(gamma)
        bt, bp = L.host_f32(beta)
        y = torch.empty_like(x)
        self._call("maa_op_layernorm_ex", L.dptr(x), rows, Cc, gp, bp, float(eps), L.dptr(y), int(out_split))
        return y

    def op_split32(self, x, slope=1.0, unpack=False):
        """x [rows, C] fp32 -> the split32 rows of leaky_relu(x, slope) (launch_split32_pack), or, with unpack, split32 rows ->
        hi + lo as fp32 (launch_split32_unpack)."""
        x = _f32(x, self.device)
        rows, Cc = x.shape
        y = torch.empty_like(x)
        self._call("maa_op_split32", L.dptr(x), rows, Cc, float(slope), int(unpack), L.dptr(y))
        return y

    def op_unfold(self, x, ks, stride):
        """maa_op_unfold: x [B, C, H, W] -> the crops [B * L, C, kh, kw] of split_input_params (torch.nn.Unfold's order)."""
        x = _f32(x, self.device)
        B, Cc, H, W = x.shape
        (kh, kw), (sh, sw) = ks, stride
        n = ((H - kh) // sh + 1) * ((W - kw) // sw + 1) if min(kh, kw, sh, sw) > 0 else 0
        y = self._empty(B * max(n, 0), Cc, kh, kw)
        self._call("maa_op_unfold", L.dptr(x), B, Cc, H, W, kh, kw, sh, sw, L.dptr(y))
        return y

    def op_fold(self, crops, weight, size, ks, stride):
        """maa_op_fold: crops [B * L, C, kh, kw], weight [kh * kw, L] -> [B, C, H, W] = fold(crops * weight) / fold(weight)."""
        crops = _f32(crops, self.device)
        (H, W), (kh, kw), (sh, sw) = size, ks, stride
        wt, wp = L.host_f32(weight)
        n = wt.shape[1]
        assert wt.shape[0] == kh * kw and crops.shape[0] % n == 0 and tuple(crops.shape[2:]) == (kh, kw)
        B, Cc = crops.shape[0] // n, crops.shape[1]
        y = self._empty(B, Cc, H, W)
        self._call("maa_op_fold", L.dptr(crops), wp, B, Cc, H, W, kh, kw, sh, sw, L.dptr(y))
        return y

    def op_conv_transpose1d(self, x, w, b, stride, leaky=0.0):
        x = _f32(x, self.device)
        B, Cin, Ln = x.shape
        _, Cout, k = w.shape
        wt, wp = L.host_f32(w)
        bt, bp = L.host_f32(b)
        y = self._empty(B, Cout, Ln * stride)
        self._call("maa_op_conv_transpose1d", L.dptr(x), B, Cin, Ln, wp, bp, Cout, k, stride, float(leaky), L.dptr(y))
        return y

    def op_mrf_pair(self, x, w1, b1, d1, slope1, w2=None, b2=None, d2=1, slope2=0.0, out_scale=1.0, out=None):
        """One MRF residual step through the generators' own dispatch.  x [B,C,L]; w1 / w2 [C,C,k] (w2 None: a ResBlock2 step);
        returns (c2(leaky(c1(leaky(x, slope1)), slope2)) + x) * out_scale, added to `out` [B,C,L] where one is given."""
        x = _f32(x, self.device)
        B, Cc, Ln = x.shape
        w1t, w1p = L.host_f32(w1)
        b1t, b1p = L.host_f32(b1) if b1 is not None else (None, None)
        w2t, w2p = L.host_f32(w2) if w2 is not None else (None, None)
        b2t, b2p = L.host_f32(b2) if b2 is not None else (None, None)
        y = _f32(out, self.device).clone() if out is not None else torch.empty_like(x)
        assert y.shape == x.shape
        self._call("maa_op_mrf_pair", L.dptr(x), B, Cc, Ln, w1p, b1p, w1.shape[2], int(d1), float(slope1), w2p, b2p,
                   w2.shape[2] if w2 is not None else 1, int(d2), float(slope2), float(out_scale), int(out is not None), L.dptr(y))
        return y

    def op_bench_conv(self, B, H, W, Cin, Cout, taps=9, pre_split=True, iters=20):
        """Kernel-only time (ms per launch) of one conv in this context's precision mode, synthetic data."""
        ms = C.c_float()
        self._call("maa_op_bench_conv", B, H, W, Cin, Cout, taps, int(pre_split), iters, C.byref(ms))
        return ms.value

    def op_snake_aa(self, x, alpha, beta, logscale):
        x = _f32(x, self.device)
        B, Cc, Ln = x.shape
        at, ap = L.host_f32(alpha)
        bt, bp = L.host_f32(beta)
        y = torch.empty_like(x)
        self._call("maa_op_snake_aa", L.dptr(x), B, Cc, Ln, ap, bp, int(logscale), L.dptr(y))
        return y


def _fill(arr, values):
    for i, v in enumerate(values):
        arr[i] = int(v)
    return len(values)


class UNet(_Handle):
    """maa_unet handle: replaces instantiate_from_config(unet_config) + load_state_dict."""

    _destroy = "maa_unet_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = cfg
        c = L.maa_unet_config()
        c.in_channels, c.out_channels, c.model_channels = cfg["in_channels"], cfg["out_channels"], cfg["model_channels"]
        c.num_res_blocks = cfg["num_res_blocks"]
        c.n_channel_mult = _fill(c.channel_mult, cfg["channel_mult"])
        c.n_attention_resolutions = _fill(c.attention_resolutions, cfg["attention_resolutions"])
        c.num_heads, c.num_head_channels = cfg["num_heads"], cfg["num_head_channels"]
        c.use_spatial_transformer = int(cfg["use_spatial_transformer"])
        c.transformer_depth = cfg.get("transformer_depth", 1)
        c.context_dim = cfg["context_dim"] or 0
        c.legacy, c.resblock_updown = int(cfg["legacy"]), int(cfg["resblock_updown"])
        c.add_context_to_emb = int(cfg.get("add_context_to_emb", False))
        self._create(ctx, "maa_unet_create", C.byref(c), state_dict=state_dict)
        self._context = None
        self._context_len = None

    def split_plan(self, split, H, W, concat=False):
        """The SplitPlan (ldm/split.py) of the reference's `split_input_params` dictionary -- or a plan already made -- for an
        [*, *, H, W] latent on this UNet; None for None.  Raises MaaError for what the reference cannot compute."""
        from .ldm import split as SP
        if split is None or isinstance(split, SP.SplitPlan):
            return split
        return SP.plan(split, H, W, down=SP.unet_down_factor(self.cfg), conditioning_key="concat" if concat else "crossattn")

    def forward_split(self, x, t, context, split):
        """One model evaluation with split_input_params (maa_unet_forward_split; ddpm_audio.py:572-654): the UNet on the
        overlapping crops of x [B, C, H, W] as one batch, stitched with the border-distance weighting.  The context's K/V are
        projected once for the B samples."""
        x = _f32(x, self.ctx.device)
        B, _, H, W = x.shape
        sp = self.split_plan(split, H, W, concat=not self.cfg["use_spatial_transformer"])
        tf = t.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        cp = None
        if context is not None:
            context = _f32(context, self.ctx.device)
            if context.dim() != 3 or context.shape[0] != B:
                raise L.MaaError("forward_split: context must be [B=%d, L, context_dim], got %s" % (B, tuple(context.shape)))
            if self._context_len != context.shape[1]:
                self.set_context(context)          # (fixes the token count the C entry reads the context with)
            cp = L.dptr(context)
        out = self._empty(B, self.cfg["out_channels"], H, W)
        wp = C.cast(sp.weight.data_ptr(), C.POINTER(C.c_float))
        self._call("maa_unet_forward_split", L.dptr(x), L.dptr(tf), cp, B, H, W, sp.kh, sp.kw, sp.sh, sp.sw, wp, L.dptr(out))
        self._context = None          # the library's context is now the tiled one: a plain forward sets its own again
        return out

    def set_context(self, context):
        """context [B, L, context_dim] on the device; K/V projections are cached for the next forwards."""
        context = _f32(context, self.ctx.device)
        self._context = context                 # keep alive: the I2A variant re-reads it every forward
        B, Ln, _ = context.shape
        self._call("maa_unet_set_context", L.dptr(context), B, Ln)
        self._context_len = Ln

    def forward(self, x, t, context=None):
        """UNetModel.forward(x, timesteps, context) (openaimodel.py:711-744)."""
        if context is not None:
            self.set_context(context)
        x = _f32(x, self.ctx.device)
        tf = t.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        out = self._empty(B, self.cfg["out_channels"], H, W)
        self._call("maa_unet_forward", L.dptr(x), L.dptr(tf), B, H, W, L.dptr(out))
        return out

    __call__ = forward

    def _ddim_args(self, what, x, timesteps, alphas, alphas_prev, cond, uncond, scale, concat, use_graph, keep, split=None):
        """maa_ddim_args for the latent x (on the device) and the S-step schedule, with the conditioning checked and kept alive in
        `keep`; `what` names the caller in the messages."""
        dev = self.ctx.device
        B, Cc, H, W = x.shape
        a = L.maa_ddim_args()
        ts = np.ascontiguousarray(np.asarray(timesteps), dtype=np.int32)
        al = np.ascontiguousarray(np.asarray(alphas), dtype=np.float32)
        ap = np.ascontiguousarray(np.asarray(alphas_prev), dtype=np.float32)
        a.S, a.B, a.C, a.H, a.W = len(ts), B, Cc, H, W
        a.scale = float(scale)
        keep += [ts, al, ap]            # (the host tables are read by the call)
        # shapes are checked here (the C ABI sees bare pointers): the reference raises from torch.cat / the attention
        # einsum on any of these mismatches (ddim.py:177-199, ddpm.py:1404-1406)
        if cond is not None:
            cond = _f32(cond, dev)
            cdim = self.cfg["context_dim"] or 0
            if cond.dim() != 3 or cond.shape[0] != B or cond.shape[2] != cdim:
                raise L.MaaError(what + ": conditioning must be [B=%d, L, %d], got %s" % (B, cdim, tuple(cond.shape)))
            keep.append(cond)
            a.d_cond = cond.data_ptr()
            a.L = cond.shape[1]
        if uncond is not None:
            if cond is None:
                raise L.MaaError(what + ": unconditional_conditioning without conditioning")
            uncond = _f32(uncond, dev)
            if tuple(uncond.shape) != tuple(cond.shape):
                raise L.MaaError(what + ": unconditional_conditioning %s must have the shape of conditioning %s"
                                 % (tuple(uncond.shape), tuple(cond.shape)))
            keep.append(uncond)
            a.d_uncond = uncond.data_ptr()
        if concat is not None:
            concat = _f32(concat, dev)
            if concat.dim() != 4 or concat.shape[0] != B or tuple(concat.shape[2:]) != (H, W) \
                    or Cc + concat.shape[1] != self.cfg["in_channels"]:
                raise L.MaaError(what + ": concat conditioning must be [B=%d, %d, %d, %d], got %s"
                                 % (B, self.cfg["in_channels"] - Cc, H, W, tuple(concat.shape)))
            keep.append(concat)
            a.d_concat = concat.data_ptr()
            a.Cc = concat.shape[1]
        a.h_timesteps = ts.ctypes.data_as(C.POINTER(C.c_int32))
        a.h_alphas = al.ctypes.data_as(C.POINTER(C.c_float))
        a.h_alphas_prev = ap.ctypes.data_as(C.POINTER(C.c_float))
        a.use_graph = int(use_graph)
        sp = self.split_plan(split, H, W, concat=concat is not None)
        if sp is not None:
            # split_input_params (ldm/split.py): crop size, stride and the host weighting [kh * kw, L]
            keep.append(sp)
            a.split_kh, a.split_kw, a.split_sh, a.split_sw = sp.kh, sp.kw, sp.sh, sp.sw
            a.h_split_weight = C.cast(sp.weight.data_ptr(), C.POINTER(C.c_float))
        self._context_len = None          # (a loop sets the library's context itself: forward_split must not trust the old length)
        return a, B, Cc, H, W

    def ddim_sample(self, x_T, timesteps, alphas, alphas_prev, cond=None, uncond=None, scale=1.0, concat=None,
                    use_graph=True, mask=None, x0=None, noise_q=None, sqrt_ac=None, sqrt_1mac=None, sigmas=None,
                    noise_p=None, temperature=1.0, log_every_t=None, split=None):
        """Whole DDIM trajectory on the device (ddim.py:118-225).  Returns x_0, or (x_0, x_inter, pred_x0) when
        log_every_t is given (the two logs as [n_log, B, C, H, W] tensors, ddim.py:158-163).
        split: the reference's `split_input_params` dictionary (or a SplitPlan of ldm/split.py): every model evaluation
        runs on overlapping crops of the latent and is stitched (ddpm_audio.py:572-654); crossattn models only.
        mask / x0 / noise_q [S, B, C, H, W] / sqrt_ac, sqrt_1mac [S]: the mask blend of ddim.py:147-150;
        sigmas [S] / noise_p [S, B, C, H, W] / temperature: the eta > 0 noise term of ddim.py:210-225.  Noise tensors
        are in loop order (first step first)."""
        return self._sample("ddim_sample", "maa_ddim_sample", x_T, timesteps, alphas, alphas_prev, cond, uncond, scale,
                            concat, use_graph, mask, x0, noise_q, sqrt_ac, sqrt_1mac, sigmas, noise_p, temperature, log_every_t,
                            split)

    def plms_sample(self, x_T, timesteps, alphas, alphas_prev, cond=None, uncond=None, scale=1.0, concat=None,
                    use_graph=True, mask=None, x0=None, noise_q=None, sqrt_ac=None, sqrt_1mac=None, log_every_t=None, split=None):
        """Whole PLMS trajectory on the device (PLMSSampler.plms_sampling, plms.py:115-236) through maa_ldm_plms_sample:
        the pseudo improved Euler step, then Adams-Bashforth steps of order up to 4; S steps make S + 1 UNet evaluations.
        Arguments and return value as ddim_sample's with eta 0 (PLMS has no noise term): the same tables, conditioning,
        mask / x0 / noise_q [S, B, C, H, W] / sqrt_ac, sqrt_1mac [S] blend before each step's first evaluation, and the logs
        of the final x_prev / pred_x0 of the logged steps; split as ddim_sample's."""
        return self._sample("plms_sample", "maa_ldm_plms_sample", x_T, timesteps, alphas, alphas_prev, cond, uncond,
                            scale, concat, use_graph, mask, x0, noise_q, sqrt_ac, sqrt_1mac, None, None, 1.0, log_every_t, split)

    def _step_noise(self, what, v, name, dim, shape, keep):
        """The device pointer of the per-step draws `v`, which must be [dim = shape[0], B, C, H, W] (`dim`: how the messages
        call the leading dimension); the tensor is kept alive in `keep`."""
        t = _f32(v, self.ctx.device)
        if tuple(t.shape) != tuple(shape):
            raise L.MaaError("%s: %s must be [%s=%d, %d, %d, %d, %d], got %s" % ((what, name, dim) + tuple(shape) + (tuple(t.shape),)))
        keep.append(t)
        return t.data_ptr()

    def _log_slabs(self, n_log, B, Cc, H, W):
        """The kept pair of [n_log, B, C, H, W] log slabs.  They are part of the captured step (their addresses are in the step
        graph's key, csrc/ddim.cpp): one pair per shape is kept by this model (four shapes at most) and the caller gets copies, so
        that a second call replays the kept graph whatever the caching allocator would have handed out for fresh tensors."""
        cache = self.__dict__.setdefault("_log_slab_cache", {})
        key = (n_log, B, Cc, H, W)
        if key not in cache:
            if len(cache) >= 4:
                cache.clear()
            cache[key] = (self._empty(*key), self._empty(*key))
        return cache[key]

    def _copy_logs(self, logs):
        """Copies of the log slabs, taken under the context's lock: the slabs are shared by every call on this model, so they are
        copied out before the lock is released, ordered behind the context's own stream (a private torch stream: copy on it; a
        library-created blocking stream orders against torch's default stream by itself, but a caller on another stream must
        wait, so drain it)."""
        dev = self.ctx.device
        if self.ctx._stream is None:
            self.ctx.synchronize()
            return logs[0].clone(), logs[1].clone()
        with torch.cuda.stream(self.ctx._stream):
            out = (logs[0].clone(), logs[1].clone())
        for t in out:
            t.record_stream(torch.cuda.current_stream(dev))
        torch.cuda.current_stream(dev).wait_stream(self.ctx._stream)
        return out

    def _sample(self, what, entry, x_T, timesteps, alphas, alphas_prev, cond, uncond, scale, concat, use_graph, mask, x0, noise_q,
                sqrt_ac, sqrt_1mac, sigmas, noise_p, temperature, log_every_t, split=None):
        """ddim_sample / plms_sample: the maa_ddim_args of a whole trajectory, the C entry `entry` on them and the logs."""
        dev = self.ctx.device
        x = _f32(x_T, dev).clone()
        keep = []
        a, B, Cc, H, W = self._ddim_args(what, x, timesteps, alphas, alphas_prev, cond, uncond, scale, concat, use_graph, keep,
                                         split)
        S = a.S

        def host_table(v, name):
            t = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
            if t.shape != (S,):
                raise L.MaaError("%s: %s must hold one value per DDIM step (%d), got %s" % (what, name, S, t.shape))
            keep.append(t)
            return t.ctypes.data_as(C.POINTER(C.c_float))

        def step_noise(v, name):
            return self._step_noise(what, v, name, "S", (S, B, Cc, H, W), keep)

        if mask is not None:
            if x0 is None or noise_q is None or sqrt_ac is None or sqrt_1mac is None:
                raise L.MaaError(what + ": mask needs x0, noise_q and the q_sample tables")      # ddim.py:148 asserts x0
            m = _f32(mask, dev).expand(B, Cc, H, W).contiguous()
            z0 = _f32(x0, dev).expand(B, Cc, H, W).contiguous()
            keep += [m, z0]
            a.d_mask, a.d_x0 = m.data_ptr(), z0.data_ptr()
            a.d_noise_q = step_noise(noise_q, "noise_q")
            a.h_sqrt_ac, a.h_sqrt_1mac = host_table(sqrt_ac, "sqrt_ac"), host_table(sqrt_1mac, "sqrt_1mac")
        if sigmas is not None:
            if noise_p is None:
                raise L.MaaError(what + ": sigmas (eta > 0) need noise_p")
            a.h_sigmas = host_table(sigmas, "sigmas")
            a.d_noise_p = step_noise(noise_p, "noise_p")
        a.temperature = float(temperature)
        logs = None
        if log_every_t is not None:
            n_log = sum(1 for i in range(S) if i % int(log_every_t) == 0 or i == S - 1)
            logs = self._log_slabs(n_log, B, Cc, H, W)
            a.log_every_t, a.n_log = int(log_every_t), n_log
            a.d_log_x, a.d_log_x0 = logs[0].data_ptr(), logs[1].data_ptr()
        with self.ctx.lock:
            self._call(entry, C.byref(a), L.dptr(x))
            if logs is not None:
                return (x,) + self._copy_logs(logs)
        return x

    def ddim_decode(self, x_latent, t_start, timesteps, alphas, alphas_prev, cond=None, uncond=None, scale=1.0, concat=None,
                    use_graph=True, sigmas=None, noise_p=None, temperature=1.0, split=None):
        """DDIMSampler.decode (ddim.py:243-261) on the device (split as ddim_sample's): the DDIM steps of indices t_start - 1 .. 0 of the S-step schedule
        (timesteps / alphas / alphas_prev as for ddim_sample) from x_latent; t_start = 0 returns a copy of x_latent.  Guidance and
        concat conditioning as for ddim_sample; sigmas [S] / noise_p [t_start, B, C, H, W] (loop order) / temperature: the eta > 0
        term.  With the same S, shapes and guidance as the last ddim_sample on this context the kept step graph is replayed."""
        dev = self.ctx.device
        x = _f32(x_latent, dev).clone()
        keep = []
        a, B, Cc, H, W = self._ddim_args("ddim_decode", x, timesteps, alphas, alphas_prev, cond, uncond, scale, concat, use_graph, keep,
                                         split)
        S = a.S
        t_start = int(t_start)
        if not 0 <= t_start <= S:
            raise L.MaaError("ddim_decode: t_start must lie in [0, S=%d], got %d" % (S, t_start))
        if sigmas is not None:
            if noise_p is None:
                raise L.MaaError("ddim_decode: sigmas (eta > 0) need noise_p")
            sg = np.ascontiguousarray(np.asarray(sigmas), dtype=np.float32)
            if sg.shape != (S,):
                raise L.MaaError("ddim_decode: sigmas must hold one value per DDIM step (%d), got %s" % (S, sg.shape))
            z = _f32(noise_p, dev)
            if tuple(z.shape) != (t_start, B, Cc, H, W):
                raise L.MaaError("ddim_decode: noise_p must be [t_start=%d, %d, %d, %d, %d], got %s"
                                 % (t_start, B, Cc, H, W, tuple(z.shape)))
            keep += [sg, z]
            a.h_sigmas = sg.ctypes.data_as(C.POINTER(C.c_float))
            a.d_noise_p = z.data_ptr() if t_start > 0 else None
        a.temperature = float(temperature)
        self._call("maa_ddim_decode", C.byref(a), t_start, L.dptr(x))
        return x

    def ddim_update(self, x, eps_uncond, eps_cond, scale, a_t, a_prev, sigma_t, sqrt_one_minus_at):
        """p_sample_ddim's elementwise tail for ONE step (ddim.py:199, 210-225 without the noise term) through
        `maa_ddim_update`: e = eu + scale (ec - eu) (eps_cond None: e = eps_uncond), returns (x_prev, pred_x0).  Used by the
        sampler's host-side loop (score correctors / callbacks); the device loop has its own fused form."""
        dev = self.ctx.device
        x, eu = _f32(x, dev), _f32(eps_uncond, dev)
        ec = None if eps_cond is None else _f32(eps_cond, dev)
        coef = torch.tensor([a_t, a_prev, sigma_t, sqrt_one_minus_at], dtype=torch.float32).to(dev)
        x_prev, pred = torch.empty_like(x), torch.empty_like(x)
        self.ctx._call("maa_ddim_update", L.dptr(x), L.dptr(eu), L.dptr(ec) if ec is not None else None, float(scale), L.dptr(coef),
                       x.numel(), L.dptr(x_prev), L.dptr(pred))
        return x_prev, pred

    # the model's schedule buffers the ancestral chain reads, under the reference's names (ddpm.py:139-155)
    DDPM_TABLES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                   "posterior_log_variance_clipped")
    DDPM_Q_TABLES = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")

    @staticmethod
    def _ddpm_tables(what, tables, names, keep):
        """Host fp32 copies of `tables[name]` (a mapping or an object with the buffers as attributes), all of one length."""
        out = []
        # (a model keeps host copies of its buffers, ldm/ddpm.py register_ancestral_schedule: no device read per call)
        host = getattr(tables, "_ddpm_host_tables", None)
        for name in names:
            if host is not None and name in host:
                v = host[name]
            else:
                v = tables[name] if isinstance(tables, dict) else getattr(tables, name)
            t = np.ascontiguousarray(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v), dtype=np.float32)
            if t.ndim != 1 or t.size == 0 or (out and t.shape != out[0].shape):
                raise L.MaaError("%s: %s must hold one fp32 value per DDPM timestep, got %s" % (what, name, t.shape))
            out.append(t)
        keep += out
        return out

    def ddpm_sample(self, x_T, tables, n=None, cond=None, uncond=None, scale=1.0, concat=None, mask=None, x0=None, noise_p=None,
                    noise_q=None, temperature=1.0, clip_denoised=True, log_every_t=None, use_graph=True, split=None, start=None):
        """The model's own ancestral (DDPM) chain on the device through maa_ddpm_sample (LatentDiffusion_audio.p_sample_loop /
        progressive_denoising, ddpm_audio.py:779-884): the steps t = start .. start - n + 1 of the schedule `tables` describes, one
        UNet evaluation and one fused kernel each.  start defaults to n - 1 (the reference's loop: t = n - 1 .. 0) and n to
        the number of timesteps.
        tables: the model's fp32 schedule buffers under the reference's names (DDPM_TABLES; with a mask DDPM_Q_TABLES too), a
        mapping or an object carrying them, one row per DDPM timestep.
        noise_p [n, B, C, H, W] (required): the steps' noise_like draws in loop order; mask / x0 / noise_q [n, B, C, H, W]: the
        blend AFTER each step with q_sample(x0, t) of the step's own t (ddpm_audio.py:873-875).  temperature: a float or one
        value per DDPM timestep (progressive_denoising's list, indexed by t).  clip_denoised: clamp x_recon to [-1, 1].
        cond / uncond / scale / concat / split / use_graph as ddim_sample's; guidance (uncond with scale != 1) is an extension,
        e = e_u + scale (e_c - e_u) -- the reference's chain evaluates the model once per step.
        Returns x_0, or (x_0, x_log, x_recon_log) when log_every_t is given: the latent after the blend and the clamped
        x_recon of every step with t % log_every_t == 0 or t == start, as [n_log, B, C, H, W] tensors in loop order."""
        what = "ddpm_sample"
        dev = self.ctx.device
        x = _f32(x_T, dev).clone()
        keep = []
        tabs = self._ddpm_tables(what, tables, self.DDPM_TABLES, keep)
        T = tabs[0].shape[0]
        n = T if n is None else int(n)
        start = n - 1 if start is None else int(start)
        if not 1 <= n <= T or not n - 1 <= start < T:
            raise L.MaaError("%s: n must lie in 1 .. %d and start in n - 1 .. %d, got n = %d, start = %d" % (what, T, T - 1, n, start))
        la, B, Cc, H, W = self._ddim_args(what, x, np.arange(T), np.ones(T), np.ones(T), cond, uncond, scale, concat, use_graph,
                                          keep, split)
        a = L.maa_ddpm_args()
        a.loop = la
        a.start, a.n, a.clip_denoised = start, n, int(bool(clip_denoised))
        fp = C.POINTER(C.c_float)
        a.h_sqrt_recip_ac, a.h_sqrt_recipm1_ac, a.h_coef1, a.h_coef2, a.h_logvar = [t.ctypes.data_as(fp) for t in tabs]

        def step_noise(v, name):
            if v is None:
                raise L.MaaError("%s: %s [n=%d, %d, %d, %d, %d] is needed" % (what, name, n, B, Cc, H, W))
            return self._step_noise(what, v, name, "n", (n, B, Cc, H, W), keep)

        a.loop.d_noise_p = step_noise(noise_p, "noise_p")
        if mask is not None:
            if x0 is None:
                raise L.MaaError(what + ": mask needs x0")          # ddpm_audio.py:860
            m = _f32(mask, dev).expand(B, Cc, H, W).contiguous()
            z0 = _f32(x0, dev).expand(B, Cc, H, W).contiguous()
            keep += [m, z0]
            a.loop.d_mask, a.loop.d_x0 = m.data_ptr(), z0.data_ptr()
            a.loop.d_noise_q = step_noise(noise_q, "noise_q")
            qt = self._ddpm_tables(what, tables, self.DDPM_Q_TABLES, keep)
            if qt[0].shape != (T,):
                raise L.MaaError("%s: the q_sample tables must hold %d rows, got %s" % (what, T, qt[0].shape))
            a.h_sqrt_ac, a.h_sqrt_1mac = [t.ctypes.data_as(fp) for t in qt]
        if np.ndim(temperature) != 0:
            tt = np.ascontiguousarray(np.asarray(temperature), dtype=np.float32)
            if tt.ndim != 1 or tt.shape[0] <= start:
                raise L.MaaError("%s: a temperature list is indexed by the timestep and must reach t = %d, got %s"
                                 % (what, start, tt.shape))
            tt = np.ascontiguousarray(np.concatenate([tt[:T], np.ones(max(0, T - tt.shape[0]), dtype=np.float32)]))
            keep.append(tt)
            a.h_temperature = tt.ctypes.data_as(fp)
        elif float(temperature) != 1.0:
            tt = np.full(T, float(temperature), dtype=np.float32)
            keep.append(tt)
            a.h_temperature = tt.ctypes.data_as(fp)
        logs = None
        if log_every_t is not None:
            every = int(log_every_t)
            if every <= 0:
                raise L.MaaError(what + ": log_every_t must be positive")
            n_log = sum(1 for t in range(start - n + 1, start + 1) if t % every == 0 or t == start)
            logs = self._log_slabs(n_log, B, Cc, H, W)
            a.loop.log_every_t, a.loop.n_log = every, n_log
            a.loop.d_log_x, a.loop.d_log_x0 = logs[0].data_ptr(), logs[1].data_ptr()
        with self.ctx.lock:
            self._call("maa_ddpm_sample", C.byref(a), L.dptr(x))
            if logs is not None:
                return (x,) + self._copy_logs(logs)
        return x

    def ddpm_update(self, x, eps, t, tables, noise, temperature=1.0, clip_denoised=True):
        """One ancestral step outside the loop (p_sample's arithmetic, ddpm_audio.py:729-777) through maa_ddpm_update:
        x_recon = sqrt_recip_ac[t] x - sqrt_recipm1_ac[t] eps (clamped when clip_denoised), the posterior mean, and
        mean + (t != 0) exp(0.5 logvar[t]) (noise temperature).  t: an int or [B] integer timesteps, one per sample, each in
        [0, num_timesteps).  Returns (x_prev, x_recon).  Used by p_sample and the host-hook loop."""
        what = "ddpm_update"
        dev = self.ctx.device
        x, eps, noise = _f32(x, dev), _f32(eps, dev), _f32(noise, dev)
        if x.dim() != 4 or eps.shape != x.shape or noise.shape != x.shape:
            raise L.MaaError("%s: x, eps and noise must share one [B, C, H, W] shape, got %s / %s / %s"
                             % (what, tuple(x.shape), tuple(eps.shape), tuple(noise.shape)))
        B, Cc, H, W = x.shape
        keep = []
        tabs = self._ddpm_tables(what, tables, self.DDPM_TABLES, keep)
        n_tab = tabs[0].shape[0]
        th = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t).reshape(-1)
        if th.size == 1:
            th = np.repeat(th, B)
        if th.shape != (B,) or not np.issubdtype(th.dtype, np.integer):
            raise L.MaaError("%s: t must hold one integer timestep per sample (B=%d), got %s %s" % (what, B, th.shape, th.dtype))
        if th.min() < 0 or th.max() >= n_tab:
            raise L.MaaError("%s: t must lie in [0, %d), got %s" % (what, n_tab, th.tolist()))
        td = torch.from_numpy(th.astype(np.int32)).to(dev)
        x_prev, x_recon = torch.empty_like(x), torch.empty_like(x)
        fp = C.POINTER(C.c_float)
        self.ctx._call("maa_ddpm_update", L.dptr(x), L.dptr(eps), C.c_void_p(td.data_ptr()),
                       *[tb.ctypes.data_as(fp) for tb in tabs], n_tab, L.dptr(noise), float(temperature), int(bool(clip_denoised)),
                       B, Cc, H, W, L.dptr(x_prev), L.dptr(x_recon))
        return x_prev, x_recon


def ddim_stochastic_encode(ctx, x0, t, sqrt_a, sqrt_1ma, noise, moments=False, scale_factor=1.0, noise_post=None):
    """DDIMSampler.stochastic_encode (ddim.py:227-241) through maa_ddim_stochastic_encode:
    out[b] = sqrt_a[t[b]] * x0[b] + sqrt_1ma[t[b]] * noise[b].  t: an int or [1] / [B] indices into the two tables
    (sqrt(ddim_alphas) / ddim_sqrt_one_minus_alphas, or the 1000-step sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod).
    moments=True: x0 is the VAE's moments [B, 2C, H, W] and the latent is formed in the same pass,
    scale_factor * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise_post) (posterior.sample() + get_first_stage_encoding)."""
    dev = ctx.device
    src = _f32(x0, dev)
    if src.dim() != 4:
        raise L.MaaError("stochastic_encode: x0 must be [B, C, H, W], got %s" % (tuple(src.shape),))
    B, C2, H, W = src.shape
    if moments:
        if C2 % 2 or noise_post is None:
            raise L.MaaError("stochastic_encode: moments must be [B, 2C, H, W] and need noise_post, got %s" % (tuple(src.shape),))
        Cc = C2 // 2
    else:
        Cc = C2
    shape = (B, Cc, H, W)
    noise = _f32(noise, dev)
    if tuple(noise.shape) != shape:
        raise L.MaaError("stochastic_encode: noise must be %s, got %s" % (shape, tuple(noise.shape)))
    npost = None
    if moments:
        npost = _f32(noise_post, dev)
        if tuple(npost.shape) != shape:
            raise L.MaaError("stochastic_encode: noise_post must be %s, got %s" % (shape, tuple(npost.shape)))
    ta = np.ascontiguousarray(np.asarray(sqrt_a.detach().cpu() if torch.is_tensor(sqrt_a) else sqrt_a), dtype=np.float32)
    tb = np.ascontiguousarray(np.asarray(sqrt_1ma.detach().cpu() if torch.is_tensor(sqrt_1ma) else sqrt_1ma), dtype=np.float32)
    if ta.ndim != 1 or ta.shape != tb.shape or ta.size == 0:
        raise L.MaaError("stochastic_encode: the two tables must be 1-D and of one length, got %s / %s" % (ta.shape, tb.shape))
    n_tab = ta.shape[0]
    th = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t).reshape(-1)
    if th.size == 1:
        th = np.repeat(th, B)
    if th.shape != (B,) or not np.issubdtype(th.dtype, np.integer):
        raise L.MaaError("stochastic_encode: t must hold one integer index per sample (B=%d), got %s %s" % (B, th.shape, th.dtype))
    if th.min() < 0 or th.max() >= n_tab:
        raise L.MaaError("stochastic_encode: t must lie in [0, %d), got %s" % (n_tab, th.tolist()))
    td = torch.from_numpy(th.astype(np.int32)).to(dev)
    out = ctx._empty(shape)
    fp = C.POINTER(C.c_float)
    ctx._call("maa_ddim_stochastic_encode", L.dptr(src), int(bool(moments)), float(scale_factor),
              L.dptr(npost) if npost is not None else None, C.c_void_p(td.data_ptr()), ta.ctypes.data_as(fp), tb.ctypes.data_as(fp),
              n_tab, L.dptr(noise), B, Cc, H, W, L.dptr(out))
    return out


class VAE(_Handle):
    _destroy = "maa_vae_destroy"

    def __init__(self, ctx, dd, state_dict):
        self.dd = dd
        c = L.maa_vae_config()
        c.ch, c.out_ch, c.in_channels, c.z_channels = dd["ch"], dd["out_ch"], dd["in_channels"], dd["z_channels"]
        c.embed_dim, c.resolution, c.num_res_blocks = dd["embed_dim"], dd["resolution"], dd["num_res_blocks"]
        c.double_z = int(dd["double_z"])
        c.n_ch_mult = _fill(c.ch_mult, dd["ch_mult"])
        c.n_attn_resolutions = _fill(c.attn_resolutions, dd["attn_resolutions"])
        self._create(ctx, "maa_vae_create", C.byref(c), state_dict=state_dict)

    def decode(self, z, scale_factor=1.0):
        """decode_first_stage (ddpm_audio.py:352-359): z [B,4,h,w] -> mel [B,1,8h,8w]."""
        z = _f32(z, self.ctx.device)
        B, _, h, w = z.shape
        f = 2 ** (len(self.dd["ch_mult"]) - 1)
        mel = self._empty(B, self.dd["out_ch"], h * f, w * f)
        self._call("maa_vae_decode", L.dptr(z), B, h, w, 1.0 / float(scale_factor), L.dptr(mel))
        return mel

    def decode_spec(self, z, scale_factor=1.0):
        """decode_first_stage + the tools' clamp((x + 1) / 2, 0, 1) in the decoder's last pass: z [B,4,h,w] -> spec [B,8h,8w]."""
        z = _f32(z, self.ctx.device)
        B, _, h, w = z.shape
        f = 2 ** (len(self.dd["ch_mult"]) - 1)
        spec = self._empty(B, h * f, w * f)
        self._call("maa_vae_decode_spec", L.dptr(z), B, h, w, 1.0 / float(scale_factor), L.dptr(spec))
        return spec

    def encode_moments(self, mel):
        """AutoencoderKL.encode moments (autoencoder.py:345-349): mel [B,1,H,W] -> [B, 2*embed, H/8, W/8]."""
        mel = _f32(mel, self.ctx.device)
        B, _, H, W = mel.shape
        f = 2 ** (len(self.dd["ch_mult"]) - 1)
        out = self._empty(B, 2 * self.dd["embed_dim"], H // f, W // f)
        self._call("maa_vae_encode_moments", L.dptr(mel), B, H, W, L.dptr(out))
        return out


class Vocoder(_Handle):
    _destroy = "maa_vocoder_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = cfg
        c = L.maa_vocoder_config()
        c.kind = 1 if cfg["kind"] == "bigvgan" else 0
        c.num_mels, c.upsample_initial_channel = cfg["num_mels"], cfg["upsample_initial_channel"]
        c.n_upsamples = _fill(c.upsample_rates, cfg["upsample_rates"])
        _fill(c.upsample_kernel_sizes, cfg["upsample_kernel_sizes"])
        c.n_kernels = _fill(c.resblock_kernel_sizes, cfg["resblock_kernel_sizes"])
        c.n_dilations = len(cfg["resblock_dilation_sizes"][0])
        for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
            for m, d in enumerate(ds):
                c.resblock_dilation_sizes[j][m] = int(d)
        c.snake_beta = int(cfg.get("activation", "") == "snakebeta")
        c.snake_logscale = int(cfg.get("snake_logscale", False))
        self.nsf = bool(cfg.get("use_pitch_embed", False))
        c.use_pitch_embed = int(self.nsf)
        c.sampling_rate = int(cfg.get("sampling_rate", 0))
        c.harmonic_num = self.harmonics = 8 if self.nsf else 0            # hifigan.py:112
        c.resblock = int(cfg.get("resblock", "1"))                        # hifigan.py:119: '1' -> ResBlock1, else ResBlock2
        if c.resblock != 1:
            c.resblock = 2
        self._create(ctx, "maa_vocoder_create", C.byref(c), state_dict=state_dict)
        self.hop = int(np.prod(cfg["upsample_rates"]))

    def forward(self, mel):
        """mel [B, num_mels, T] -> wav [B, 1, T*hop] (HifiGanGenerator.forward, hifigan.py:144-169)."""
        mel = _f32(mel, self.ctx.device)
        B, _, T = mel.shape
        wav = self._empty(B, 1, T * self.hop)
        self._call("maa_vocoder_forward", L.dptr(mel), B, T, L.dptr(wav))
        return wav

    def forward_f0(self, mel, f0, rand_ini=None, noise=None):
        """NSF branch (HifiGanGenerator.forward(x, f0), hifigan.py:144-157): mel [B, num_mels, T], f0 [B, T] in Hz.
        rand_ini [B, 9] / noise [B, T*hop, 9] are the two tensors SineGen.forward draws (source.py:355-358, 425); when
        omitted they are drawn here with torch's global generator in the reference's order and on the mel's device."""
        if not self.nsf:
            raise L.MaaError("this generator has no NSF branch (use_pitch_embed is off)")
        dev = self.ctx.device
        mel, f0 = _f32(mel, dev), _f32(f0, dev)
        B, _, T = mel.shape
        if tuple(f0.shape) != (B, T):
            raise L.MaaError("forward_f0: f0 must be [B=%d, T=%d], got %s" % (B, T, tuple(f0.shape)))
        H1, Ln = self.harmonics + 1, T * self.hop
        if rand_ini is None:
            rand_ini = torch.rand(B, H1, device=dev)
        if noise is None:
            noise = torch.randn(B, Ln, H1, device=dev)
        rand_ini, noise = _f32(rand_ini, dev), _f32(noise, dev)
        if tuple(rand_ini.shape) != (B, H1) or tuple(noise.shape) != (B, Ln, H1):
            raise L.MaaError("forward_f0: rand_ini must be [%d, %d] and noise [%d, %d, %d]" % (B, H1, B, Ln, H1))
        wav = self._empty(B, 1, Ln)
        self._call("maa_vocoder_forward_f0", L.dptr(mel), L.dptr(f0), L.dptr(rand_ini), L.dptr(noise), B, T, L.dptr(wav))
        return wav

    def __call__(self, mel, f0=None, **kw):
        return self.forward(mel) if f0 is None else self.forward_f0(mel, f0, **kw)


class DiffNet(_Handle):
    """maa_diffnet handle: DiffSinger's denoiser (NeuralSeq/modules/diff/net.py:84-130) and the PLMS loop over it
    (NeuralSeq/modules/diff/shallow_diffusion_tts.py:166-201, 262-269)."""

    _destroy = "maa_diffnet_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = cfg
        c = L.maa_diffnet_config()
        c.in_dims, c.hidden_size = cfg["in_dims"], cfg["hidden_size"]
        c.residual_layers, c.residual_channels = cfg["residual_layers"], cfg["residual_channels"]
        c.dilation_cycle_length = cfg["dilation_cycle_length"]
        self._create(ctx, "maa_diffnet_create", C.byref(c), state_dict=state_dict)

    def forward(self, spec, diffusion_step, cond):
        """spec [B, 1, M, T], diffusion_step [B] or [B, 1] (integer steps), cond [B, H, T] -> eps [B, 1, M, T]."""
        dev = self.ctx.device
        spec, cond = _f32(spec, dev), _f32(cond, dev)
        t = _f32(torch.as_tensor(diffusion_step).reshape(-1), dev)
        B, _, M, T = spec.shape
        if M != self.cfg["in_dims"] or tuple(cond.shape) != (B, self.cfg["hidden_size"], T) or t.shape[0] != B:
            raise L.MaaError("DiffNet.forward: spec %s / step %s / cond %s do not fit in_dims %d, hidden_size %d"
                             % (tuple(spec.shape), tuple(t.shape), tuple(cond.shape), self.cfg["in_dims"], self.cfg["hidden_size"]))
        out = torch.empty_like(spec)
        self._call("maa_diffnet_forward", L.dptr(spec), L.dptr(t), L.dptr(cond), B, T, L.dptr(out))
        return out

    __call__ = forward

    def plms_sample(self, x, cond, alphas_cumprod, K_step, interval, use_graph=True):
        """x [B, 1, M, T] = x_K -> x_0 after the pndm_speedup loop: t = K_step - interval, ..., 0."""
        dev = self.ctx.device
        x = _f32(x, dev).clone()
        cond = _f32(cond, dev)
        B, _, M, T = x.shape
        if M != self.cfg["in_dims"] or tuple(cond.shape) != (B, self.cfg["hidden_size"], T):
            raise L.MaaError("plms_sample: x %s / cond %s do not fit the denoiser" % (tuple(x.shape), tuple(cond.shape)))
        if B > 256:
            raise L.MaaError("plms_sample: at most 256 samples per call (got %d)" % B)
        ac = np.ascontiguousarray(np.asarray(alphas_cumprod), dtype=np.float32)
        a = L.maa_plms_args()
        a.B, a.T, a.K_step, a.interval, a.timesteps = B, T, int(K_step), int(interval), int(ac.shape[0])
        a.d_cond = cond.data_ptr()
        a.h_alphas_cumprod = ac.ctypes.data_as(C.POINTER(C.c_float))
        a.use_graph = int(use_graph)
        self._call("maa_plms_sample", C.byref(a), L.dptr(x))
        return x

    @staticmethod
    def _ddpm_tables(what, tables):
        """The five host tables of the ancestral step, fp32 and of one length: (sqrt_recip_alphas_cumprod,
        sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2, sigma)."""
        if len(tables) != 5:
            raise L.MaaError(what + ": tables = (sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sigma), got %d" % len(tables))
        tabs = [np.ascontiguousarray(np.asarray(t), dtype=np.float32).reshape(-1) for t in tables]
        if tabs[0].shape[0] < 1 or any(t.shape[0] != tabs[0].shape[0] for t in tabs):
            raise L.MaaError(what + ": the tables need one row per timestep each, got %s" % [t.shape[0] for t in tabs])
        return tabs, [t.ctypes.data_as(C.POINTER(C.c_float)) for t in tabs]

    def ddpm_sample(self, x, cond, tables, start, n, noise, clip_denoised=True, use_graph=True):
        """The ancestral steps t = start, ..., start - n + 1 on the device through maa_ds_ddpm_sample (p_sample in the loop of
        shallow_diffusion_tts.py:269-271): x [B, 1, M, T] at step `start` -> x after step start - n + 1 (a new tensor).
        tables: see _ddpm_tables; noise [n, B, 1, M, T]: the steps' draws in loop order."""
        what = "ds_ddpm_sample"
        dev = self.ctx.device
        x = _f32(x, dev).clone()
        cond, noise = _f32(cond, dev), _f32(noise, dev)
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] != self.cfg["in_dims"]:
            raise L.MaaError("%s: x %s is not [B, 1, %d, T]" % (what, tuple(x.shape), self.cfg["in_dims"]))
        B, _, M, T = x.shape
        if tuple(cond.shape) != (B, self.cfg["hidden_size"], T):
            raise L.MaaError("%s: cond %s does not fit x %s: it must be [B, %d, T]"
                             % (what, tuple(cond.shape), tuple(x.shape), self.cfg["hidden_size"]))
        if B > 256:
            raise L.MaaError("%s: at most 256 samples per call (got %d)" % (what, B))
        start, n = int(start), int(n)
        tabs, ptrs = self._ddpm_tables(what, tables)
        if n < 1:
            raise L.MaaError("%s: the number of steps n must be at least 1 (got %d)" % (what, n))
        if start < 0 or start >= tabs[0].shape[0]:
            raise L.MaaError("%s: start %d lies outside the schedule of %d timesteps" % (what, start, tabs[0].shape[0]))
        if start - n + 1 < 0:
            raise L.MaaError("%s: %d steps from t = %d run past t = 0" % (what, n, start))
        if tuple(noise.shape) != (n,) + tuple(x.shape):
            raise L.MaaError("%s: noise %s is not [n = %d] + x %s" % (what, tuple(noise.shape), n, tuple(x.shape)))
        a = L.maa_ds_ddpm_args()
        a.B, a.T, a.start, a.n, a.timesteps = B, T, start, n, int(tabs[0].shape[0])
        a.clip_denoised, a.use_graph = int(bool(clip_denoised)), int(bool(use_graph))
        a.d_cond, a.d_noise = cond.data_ptr(), noise.data_ptr()
        a.h_sqrt_recip_ac, a.h_sqrt_recipm1_ac, a.h_coef1, a.h_coef2, a.h_sigma = ptrs
        self._call("maa_ds_ddpm_sample", C.byref(a), L.dptr(x))
        return x

    def ddpm_update(self, x, eps, t, tables, noise, clip_denoised=True):
        """One ancestral step outside the loop through maa_ds_ddpm_update (p_sample's arithmetic after the denoiser,
        shallow_diffusion_tts.py:134-166): x, eps, noise [B, 1, M, T], t [B] integer steps (one per sample) -> x_{t-1} (new)."""
        what = "ds_ddpm_update"
        dev = self.ctx.device
        x = _f32(x, dev).clone()
        eps, noise = _f32(eps, dev), _f32(noise, dev)
        t = _f32(torch.as_tensor(t).reshape(-1), dev)
        if x.dim() != 4 or x.shape[1] != 1 or eps.shape != x.shape or noise.shape != x.shape or t.shape[0] != x.shape[0]:
            raise L.MaaError("%s: x %s / eps %s / noise %s / t %s do not fit each other"
                             % (what, tuple(x.shape), tuple(eps.shape), tuple(noise.shape), tuple(t.shape)))
        B, _, M, T = x.shape
        tabs, ptrs = self._ddpm_tables(what, tables)
        self.ctx._call("maa_ds_ddpm_update", L.dptr(eps), L.dptr(t), L.dptr(noise), *ptrs, int(tabs[0].shape[0]), B, M, T,
                       int(bool(clip_denoised)), L.dptr(x))
        return x


def pe_config(cfg):
    """maa_pitch_extractor_config of a PitchExtractor hparams dict (config.PITCH_EXTRACTOR); refuses what the library does not
    build, with the reason, before any device is touched."""
    pad = cfg.get("ffn_padding", "SAME")
    if pad != "SAME":
        raise L.MaaError("PitchExtractor: ffn_padding %r is not supported: only 'SAME' (kernel // 2 zeros on both sides) is built, "
                         "the causal 'LEFT' padding (kernel - 1, 0) is not" % (pad,))
    norm = cfg.get("pitch_norm", "log")
    if norm not in ("log", "standard"):
        raise L.MaaError("PitchExtractor: pitch_norm %r: the reference has 'log' and 'standard'" % (norm,))
    if cfg.get("pitch_type", "frame") != "frame":
        raise L.MaaError("PitchExtractor: pitch_type %r is not supported: only 'frame'" % (cfg.get("pitch_type"),))
    c = L.maa_pitch_extractor_config()
    c.n_mel_bins, c.hidden_size = int(cfg["n_mel_bins"]), int(cfg["hidden_size"])
    c.predictor_hidden, c.predictor_kernel = int(cfg.get("predictor_hidden", -1)), int(cfg.get("predictor_kernel", 5))
    c.conv_layers = int(cfg.get("conv_layers", 2))
    c.ffn_padding_same = 1
    c.use_uv = int(bool(cfg.get("use_uv", True)))          # (pitch_type == 'frame' holds here)
    c.pitch_norm = 0 if norm == "log" else 1
    c.f0_mean, c.f0_std = float(cfg.get("f0_mean", 0.0)), float(cfg.get("f0_std", 1.0))
    return c


class PitchExtractor(_Handle):
    """maa_pitch_extractor handle: DiffSinger's PitchExtractor (NeuralSeq/modules/fastspeech/pe.py:119-149), mel -> f0."""

    _destroy = "maa_pitch_extractor_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = dict(cfg)
        self._create(ctx, "maa_pitch_extractor_create", C.byref(pe_config(self.cfg)), state_dict=state_dict)

    def forward(self, mel, return_hidden=False):
        """mel [B, T, n_mel_bins] (an all-zero frame is padding) -> (pitch_pred [B, T, 2], f0 [B, T]) on the device; with
        return_hidden also mel_hidden [B, T, hidden_size], the input of pitch_predictor."""
        mel = _f32(mel, self.ctx.device)
        if mel.dim() != 3 or mel.shape[2] != self.cfg["n_mel_bins"] or mel.shape[0] < 1 or mel.shape[1] < 1:
            raise L.MaaError("PitchExtractor.forward: mel %s is not [B, T, %d]" % (tuple(mel.shape), self.cfg["n_mel_bins"]))
        B, T, _ = mel.shape
        pitch_pred = self._empty(B, T, 2)
        f0 = self._empty(B, T)
        hidden = self._empty(B, T, self.cfg["hidden_size"]) if return_hidden else None
        self._call("maa_pitch_extractor_forward", L.dptr(mel), B, T, L.dptr(pitch_pred), L.dptr(f0),
                   L.dptr(hidden) if return_hidden else None)
        return (pitch_pred, f0, hidden) if return_hidden else (pitch_pred, f0)

    __call__ = forward


GLOW_FIELDS = ("in_channels", "hidden_channels", "kernel_size", "dilation_rate", "n_blocks", "n_layers", "n_split", "n_sqz",
               "gin_channels", "share_cond_layers", "share_wn_layers", "sigmoid_scale")


def glow_config(cfg):
    """maa_glow_config of a Glow hparams dict (config.GENERSPEECH_POST_GLOW); refuses what the library does not build, with the
    reason, before any device is touched.  p_dropout is not read (eval)."""
    kind = cfg.get("inv_conv_type", "near")
    if kind != "near":
        raise L.MaaError("Glow: inv_conv_type %r is not supported: only 'near' (InvConvNear, the 4 x 4 mix over channel groups) "
                         "is built, the full-width 'invconv' is not" % (kind,))
    if int(cfg.get("n_sqz", 2)) != 2:
        raise L.MaaError("Glow: n_sqz %r is not supported: the squeeze is built as the pairing of neighbouring frames (n_sqz 2) "
                         "only" % (cfg.get("n_sqz"),))
    if int(cfg.get("n_split", 4)) != 4:
        raise L.MaaError("Glow: n_split %r is not supported: InvConvNear is built as the 4 x 4 mix (n_split 4) only" % (cfg.get("n_split"),))
    if int(cfg["kernel_size"]) < 1 or int(cfg["kernel_size"]) % 2 == 0:
        raise L.MaaError("Glow: kernel_size %r must be odd: WN asserts it ('same' padding keeps the length only then)" % (cfg["kernel_size"],))
    if int(cfg["hidden_channels"]) < 2 or int(cfg["hidden_channels"]) % 2 != 0:
        raise L.MaaError("Glow: hidden_channels %r must be even: WN asserts it" % (cfg["hidden_channels"],))
    if int(cfg["hidden_channels"]) % 4 != 0:
        raise L.MaaError("Glow: hidden_channels %r must be a multiple of 4: the row kernels move 16 bytes per lane" % (cfg["hidden_channels"],))
    if int(cfg["in_channels"]) < 4 or int(cfg["in_channels"]) % 4 != 0:
        raise L.MaaError("Glow: in_channels %r: in_channels %% 4 != 0 -- the row kernels move 16 bytes per lane and the 4 x 4 mix stays "
                         "inside a lane" % (cfg["in_channels"],))
    if int(cfg.get("gin_channels", 0)) < 0 or int(cfg.get("gin_channels", 0)) % 4 != 0:
        raise L.MaaError("Glow: gin_channels %r must be 0 (no conditioning) or a multiple of 4" % (cfg.get("gin_channels"),))
    c = L.maa_glow_config()
    for k in GLOW_FIELDS:
        setattr(c, k, int(cfg.get(k, {"n_split": 4, "n_sqz": 2, "dilation_rate": 1}.get(k, 0))))
    return c


class Glow(_Handle):
    """maa_glow handle: the Glow post-net in reverse (NeuralSeq/modules/GenerSpeech/model/glow_modules.py:496-580) on channels-last
    rows."""

    _destroy = "maa_glow_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = dict(cfg)
        self._create(ctx, "maa_glow_create", C.byref(glow_config(self.cfg)), state_dict=state_dict)

    def reverse(self, z, g=None, mask=None, return_logdet=True, return_hiddens=False):
        """z [B, T, in_channels], g [B, T, gin_channels] (None exactly when gin_channels == 0), mask [B, T] of 0 / 1 (None: all
        ones) -> (x [B, 2 (T // 2), in_channels], logdet [B] or None, hiddens [3 n_blocks, B, T // 2, 2 in_channels] or None)."""
        Cc, gin = self.cfg["in_channels"], self.cfg["gin_channels"]
        z = _f32(z, self.ctx.device)
        if z.dim() != 3 or z.shape[2] != Cc or z.shape[0] < 1:
            raise L.MaaError("Glow.reverse: z %s is not [B, T, %d]" % (tuple(z.shape), Cc))
        B, T, _ = z.shape
        if T < 2:
            raise L.MaaError("Glow.reverse: T < 2 -- the squeeze pairs frames, T = %d leaves no row" % T)
        if (g is None) != (gin == 0):
            raise L.MaaError("Glow.reverse: g must be given exactly when gin_channels > 0 (gin_channels = %d)" % gin)
        if g is not None:
            g = _f32(g, self.ctx.device)
            if tuple(g.shape) != (B, T, gin):
                raise L.MaaError("Glow.reverse: g %s is not [%d, %d, %d]" % (tuple(g.shape), B, T, gin))
        if mask is not None:
            mask = _f32(mask, self.ctx.device)
            if tuple(mask.shape) != (B, T):
                raise L.MaaError("Glow.reverse: mask %s is not [%d, %d]" % (tuple(mask.shape), B, T))
        Ts = T // 2
        x = self._empty(B, 2 * Ts, Cc)
        logdet = self._empty(B) if return_logdet else None
        hs = self._empty(3 * self.cfg["n_blocks"], B, Ts, 2 * Cc) if return_hiddens else None
        p = lambda t: L.dptr(t) if t is not None else None          # noqa: E731
        self._call("maa_glow_reverse", L.dptr(z), p(g), p(mask), B, T, L.dptr(x), p(logdet), p(hs))
        return x, logdet, hs


def fs2_config(cfg):
    """maa_fs2_config of a FastSpeech2MIDI hparams dict (config.FASTSPEECH2_MIDI); refuses what the library does not build, with
    the reason, before any device is touched."""
    if cfg.get("use_pitch_embed", False):
        raise L.MaaError("FastSpeech2MIDI: use_pitch_embed is not supported by this handle: the pitch branch is FS2Pitch beside "
                         "it, composed by diffsinger.FastSpeech2MIDICascade")
    for k in ("use_energy_embed", "use_spk_id", "use_spk_embed", "use_bert"):
        if cfg.get(k, False):
            raise L.MaaError("FastSpeech2MIDI: %s is not supported: no shipped e2e singing configuration sets it and its branch "
                             "is not built" % k)
    for k in ("rel_pos", "use_pos_embed"):
        if not cfg.get(k, k == "use_pos_embed"):
            raise L.MaaError("FastSpeech2MIDI: %s must be true: the encoder's positions are RelPositionalEncoding, the only form "
                             "built" % k)
    pad = cfg.get("ffn_padding", "SAME")
    if pad != "SAME":
        raise L.MaaError("FastSpeech2MIDI: ffn_padding %r is not supported: only 'SAME' (kernel // 2 zeros on both sides) is built, "
                         "the causal 'LEFT' padding (kernel - 1, 0) is not" % (pad,))
    if cfg.get("ffn_act", "gelu") != "gelu":
        raise L.MaaError("FastSpeech2MIDI: ffn_act %r is not supported: only 'gelu' is built into the FFN's epilogue" % (cfg.get("ffn_act"),))
    if cfg.get("dur_loss", "mse") != "mse":
        raise L.MaaError("FastSpeech2MIDI: dur_loss %r is not supported: only 'mse' (round(exp(x) - 1)) is built" % (cfg.get("dur_loss"),))
    for k in ("encoder_type", "decoder_type"):
        if cfg.get(k, "fft") != "fft":
            raise L.MaaError("FastSpeech2MIDI: %s %r is not supported: only 'fft' (FFTBlocks) is built" % (k, cfg.get(k)))
    H, nh = int(cfg["hidden_size"]), int(cfg["num_heads"])
    if nh < 1 or H != 128 * nh:
        raise L.MaaError("FastSpeech2MIDI: hidden_size %d / num_heads %d is not 128, the only head width the masked attention is "
                         "built and tested for" % (H, nh))
    c = L.maa_fs2_config()
    for k in ("vocab_size", "hidden_size", "enc_layers", "dec_layers", "num_heads", "enc_ffn_kernel_size", "dec_ffn_kernel_size",
              "audio_num_mel_bins"):
        setattr(c, k, int(cfg[k]))
    c.dur_predictor_layers, c.dur_predictor_kernel = int(cfg.get("dur_predictor_layers", 5)), int(cfg.get("dur_predictor_kernel", 3))
    c.predictor_hidden = int(cfg.get("predictor_hidden", -1))
    c.ffn_padding_same = c.ffn_act_gelu = c.dur_loss_mse = c.rel_pos = c.use_pos_embed = c.encoder_fft = c.decoder_fft = 1
    return c


class FastSpeech2MIDI(_Handle):
    """maa_fs2 handle: DiffSinger's FastSpeech2MIDI front end (NeuralSeq/modules/diffsinger_midi/fs2.py:46-118).  Integer tensors
    cross the boundary as int32; nothing here reads the device."""

    _destroy = "maa_fs2_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = dict(cfg)
        self._create(ctx, "maa_fs2_create", C.byref(fs2_config(self.cfg)), state_dict=state_dict)

    def _i32(self, t):
        return torch.as_tensor(t).to(device=self.ctx.device, dtype=torch.int32).contiguous()

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def encode(self, txt_tokens, pitch_midi, midi_dur=None, is_slur=None):
        """[B, T] tokens and note features -> (encoder_out [B, T, H], xs [B, T], dur int32 [B, T], totals int32 [B])."""
        tok, midi = self._i32(txt_tokens), self._i32(pitch_midi)
        B, T = tok.shape
        dur_f = _f32(midi_dur, self.ctx.device) if midi_dur is not None else None
        slur = self._i32(is_slur) if is_slur is not None else None
        for name, t in (("pitch_midi", midi), ("midi_dur", dur_f), ("is_slur", slur)):
            if t is not None and tuple(t.shape) != (B, T):
                raise L.MaaError("FastSpeech2MIDI.encode: %s %s is not txt_tokens' [%d, %d]" % (name, tuple(t.shape), B, T))
        dev = self.ctx.device
        enc = self._empty(B, T, self.cfg["hidden_size"])
        xs = self._empty(B, T)
        dur = self._empty(B, T, dtype=torch.int32)
        totals = self._empty(B, dtype=torch.int32)
        self._call("maa_fs2_encode", self._p(tok), self._p(midi), self._p(dur_f), self._p(slur), B, T, self._p(enc), self._p(xs),
                   self._p(dur), self._p(totals))
        return enc, xs, dur, totals

    def length_regulate(self, dur, T_mel):
        """dur int32 [B, T] -> mel2ph int32 [B, T_mel]."""
        dur = self._i32(dur)
        B, T = dur.shape
        mel2ph = self._empty(B, int(T_mel), dtype=torch.int32)
        self._call("maa_fs2_length_regulate", self._p(dur), B, T, int(T_mel), self._p(mel2ph))
        return mel2ph

    def decode(self, encoder_out, mel2ph, skip_decoder=False):
        """encoder_out [B, T, H], mel2ph [B, T_mel] -> (decoder_inp [B, T_mel, H], mel_out [B, T_mel, mel bins] or None)."""
        enc = _f32(encoder_out, self.ctx.device)
        m2p = self._i32(mel2ph)
        B, T, _ = enc.shape
        if m2p.dim() != 2 or m2p.shape[0] != B or m2p.shape[1] < 1:
            raise L.MaaError("FastSpeech2MIDI.decode: mel2ph %s is not [%d, T_mel]" % (tuple(m2p.shape), B))
        T_mel = int(m2p.shape[1])
        dev = self.ctx.device
        dec_inp = self._empty(B, T_mel, self.cfg["hidden_size"])
        mel = None if skip_decoder else self._empty(B, T_mel, self.cfg["audio_num_mel_bins"])
        self._call("maa_fs2_decode", self._p(enc), self._p(m2p), B, T, T_mel, self._p(dec_inp), self._p(mel))
        return dec_inp, mel

    def run_decoder(self, decoder_inp, mel2ph):
        """FastSpeech2.run_decoder: decoder_inp [B, T_mel, H] (an all-zero row is padding), mel2ph [B, T_mel] -> mel_out
        [B, T_mel, mel bins]: decode's second half on a decoder_inp another stage finished (FS2Pitch)."""
        x = _f32(decoder_inp, self.ctx.device)
        m2p = self._i32(mel2ph)
        if x.dim() != 3 or x.shape[2] != self.cfg["hidden_size"] or x.shape[0] < 1 or x.shape[1] < 1:
            raise L.MaaError("FastSpeech2MIDI.run_decoder: decoder_inp %s is not [B, T_mel, %d]" % (tuple(x.shape), self.cfg["hidden_size"]))
        B, T_mel, _ = x.shape
        if tuple(m2p.shape) != (B, T_mel):
            raise L.MaaError("FastSpeech2MIDI.run_decoder: mel2ph %s is not [%d, %d]" % (tuple(m2p.shape), B, T_mel))
        mel = self._empty(B, T_mel, self.cfg["audio_num_mel_bins"])
        self._call("maa_fs2_run_decoder", self._p(x), self._p(m2p), B, T_mel, self._p(mel))
        return mel


def fs2_plain_config(cfg):
    """maa_fs2_config (plain = 1) of a plain FastSpeech2 hparams dict (config.FASTSPEECH2) with use_pitch_embed cleared -- the
    pitch branch is FS2Pitch beside the handle; refuses what the library does not build, with the reason, before any device is
    touched."""
    what = "FastSpeech2"
    if cfg.get("use_pitch_embed", False):
        raise L.MaaError("%s: use_pitch_embed is not supported by this handle: the pitch branch is FS2Pitch beside it, composed by "
                         "diffsinger.FastSpeech2" % what)
    if cfg.get("use_bert", False):
        raise L.MaaError("%s: use_bert is not supported: BERTRelTransformerEncoder and its word-level features are not built" % what)
    if not cfg.get("use_pos_embed", True):
        raise L.MaaError("%s: use_pos_embed must be true: an encoder without positions is not built" % what)
    if cfg.get("use_spk_id", False) and cfg.get("use_spk_embed", False):
        raise L.MaaError("%s: use_spk_id and use_spk_embed are alternatives (the reference takes use_spk_id when both are set): "
                         "set one" % what)
    if cfg.get("use_split_spk_id", False) and not cfg.get("use_spk_id", False):
        raise L.MaaError("%s: use_split_spk_id without use_spk_id: the reference builds no table for it" % what)
    if cfg.get("use_spk_id", False) and int(cfg.get("num_spk", 0)) < 1:
        raise L.MaaError("%s: use_spk_id needs num_spk >= 1 (the tables have num_spk + 1 rows)" % what)
    pad = cfg.get("ffn_padding", "SAME")
    if pad != "SAME":
        raise L.MaaError("%s: ffn_padding %r is not supported: only 'SAME' (kernel // 2 zeros on both sides) is built, "
                         "the causal 'LEFT' padding (kernel - 1, 0) is not" % (what, pad))
    if cfg.get("ffn_act", "gelu") != "gelu":
        raise L.MaaError("%s: ffn_act %r is not supported: only 'gelu' is built into the FFN's epilogue" % (what, cfg.get("ffn_act")))
    if cfg.get("dur_loss", "mse") != "mse":
        raise L.MaaError("%s: dur_loss %r is not supported: only 'mse' (round(exp(x) - 1)) is built" % (what, cfg.get("dur_loss")))
    for k in ("encoder_type", "decoder_type"):
        if cfg.get(k, "fft") != "fft":
            raise L.MaaError("%s: %s %r is not supported: only 'fft' (FFTBlocks) is built" % (what, k, cfg.get(k)))
    H, nh = int(cfg["hidden_size"]), int(cfg["num_heads"])
    if nh < 1 or H != 128 * nh:
        raise L.MaaError("%s: hidden_size %d / num_heads %d is not 128, the only head width the masked attention is "
                         "built and tested for" % (what, H, nh))
    c = L.maa_fs2_config()
    for k in ("vocab_size", "hidden_size", "enc_layers", "dec_layers", "num_heads", "enc_ffn_kernel_size", "dec_ffn_kernel_size",
              "audio_num_mel_bins"):
        setattr(c, k, int(cfg[k]))
    c.dur_predictor_layers, c.dur_predictor_kernel = int(cfg.get("dur_predictor_layers", 5)), int(cfg.get("dur_predictor_kernel", 3))
    c.predictor_hidden = int(cfg.get("predictor_hidden", -1))
    c.predictor_layers, c.predictor_kernel = int(cfg.get("predictor_layers", 5)), int(cfg.get("predictor_kernel", 5))
    c.ffn_padding_same = c.ffn_act_gelu = c.dur_loss_mse = c.use_pos_embed = c.encoder_fft = c.decoder_fft = c.plain = 1
    c.rel_pos = int(bool(cfg.get("rel_pos", False)))
    c.use_energy_embed = int(bool(cfg.get("use_energy_embed", False)))
    c.use_spk_id, c.use_spk_embed = int(bool(cfg.get("use_spk_id", False))), int(bool(cfg.get("use_spk_embed", False)))
    c.use_split_spk_id = int(bool(cfg.get("use_split_spk_id", False)))
    c.num_spk = int(cfg.get("num_spk", 0)) if c.use_spk_id else 0
    return c


class FastSpeech2Plain(FastSpeech2MIDI):
    """maa_fs2 handle created with plain = 1: the reference's plain FastSpeech2 (NeuralSeq/modules/fastspeech/fs2.py) without its
    pitch branch.  length_regulate, decode and run_decoder are FastSpeech2MIDI's; nothing here reads the device."""

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = dict(cfg)
        self._create(ctx, "maa_fs2_create", C.byref(fs2_plain_config(self.cfg)), state_dict=state_dict)

    def encode(self, txt_tokens, spk_dur=None):
        """[B, T] tokens, spk_dur [B, H] or None -> (encoder_out [B, T, H], xs [B, T], dur int32 [B, T], totals int32 [B])."""
        tok = self._i32(txt_tokens)
        B, T = tok.shape
        H = self.cfg["hidden_size"]
        spk_dur = _f32(spk_dur, self.ctx.device) if spk_dur is not None else None
        if spk_dur is not None and tuple(spk_dur.shape) != (B, H):
            raise L.MaaError("FastSpeech2Plain.encode: spk_dur %s is not [%d, %d]" % (tuple(spk_dur.shape), B, H))
        enc = self._empty(B, T, H)
        xs = self._empty(B, T)
        dur = self._empty(B, T, dtype=torch.int32)
        totals = self._empty(B, dtype=torch.int32)
        self._call("maa_fs2_encode_plain", self._p(tok), self._p(spk_dur), B, T, self._p(enc), self._p(xs), self._p(dur),
                   self._p(totals))
        return enc, xs, dur, totals

    def speaker(self, ids=None, vec=None):
        """ids int [3, B] (speaker, dur, f0 ids) for a use_spk_id handle, vec [B, 256] for a use_spk_embed one -> [3, B, H]:
        spk_embed, spk_embed_dur, spk_embed_f0."""
        if ids is None and vec is None:
            raise L.MaaError("FastSpeech2Plain.speaker: neither ids nor vec")
        ids = self._i32(ids) if ids is not None else None
        vec = _f32(vec, self.ctx.device) if vec is not None else None
        if ids is not None and (ids.dim() != 2 or ids.shape[0] != 3 or ids.shape[1] < 1):
            raise L.MaaError("FastSpeech2Plain.speaker: ids %s is not [3, B]" % (tuple(ids.shape),))
        if vec is not None and (vec.dim() != 2 or vec.shape[1] != 256 or vec.shape[0] < 1):
            raise L.MaaError("FastSpeech2Plain.speaker: vec %s is not [B, 256]" % (tuple(vec.shape),))
        B = int(ids.shape[1] if ids is not None else vec.shape[0])
        if ids is not None and vec is not None and vec.shape[0] != B:
            raise L.MaaError("FastSpeech2Plain.speaker: ids and vec disagree on B")
        out = self._empty(3, B, self.cfg["hidden_size"])
        self._call("maa_fs2_speaker", self._p(ids), self._p(vec), B, self._p(out))
        return out

    def _frames(self, what, x, mel2ph):
        x = _f32(x, self.ctx.device)
        m2p = self._i32(mel2ph)
        if x.dim() != 3 or x.shape[2] != self.cfg["hidden_size"] or x.shape[0] < 1 or x.shape[1] < 1:
            raise L.MaaError("FastSpeech2Plain.%s: %s is not [B, T_mel, %d]" % (what, tuple(x.shape), self.cfg["hidden_size"]))
        if tuple(m2p.shape) != tuple(x.shape[:2]):
            raise L.MaaError("FastSpeech2Plain.%s: mel2ph %s is not %s" % (what, tuple(m2p.shape), tuple(x.shape[:2])))
        return x, m2p

    def _spk(self, what, spk, B):
        if spk is None:
            return None
        spk = _f32(spk, self.ctx.device)
        if tuple(spk.shape) != (B, self.cfg["hidden_size"]):
            raise L.MaaError("FastSpeech2Plain.%s: the speaker vector %s is not [%d, %d]" % (what, tuple(spk.shape), B, self.cfg["hidden_size"]))
        return spk

    def add_speaker(self, x, spk, mel2ph):
        """(x [B, T_mel, H] + spk [B, H]) * (mel2ph > 0): the pitch and energy predictors' input."""
        x, m2p = self._frames("add_speaker", x, mel2ph)
        B, T_mel, H = x.shape
        out = self._empty(B, T_mel, H)
        self._call("maa_fs2_add_speaker", self._p(x), self._p(self._spk("add_speaker", spk, B)), self._p(m2p), B, T_mel, self._p(out))
        return out

    def finish(self, pred_inp, acc, mel2ph, energy=None, spk=None, return_bin=False):
        """The energy branch (when the handle has one) on pred_inp, then decoder_inp = (acc + energy_embed[bin] + spk[b]) *
        (mel2ph > 0) -> (decoder_inp [B, T_mel, H], energy_pred [B, T_mel] or None[, energy_bin int32 [B, T_mel] or None])."""
        acc, m2p = self._frames("finish", acc, mel2ph)
        B, T_mel, H = acc.shape
        has = bool(self.cfg.get("use_energy_embed", False))
        pred_inp = self._frames("finish", pred_inp, m2p)[0] if has else None
        energy = _f32(energy, self.ctx.device) if energy is not None and has else None
        if energy is not None and tuple(energy.shape) != (B, T_mel):
            raise L.MaaError("FastSpeech2Plain.finish: energy %s is not [%d, %d]" % (tuple(energy.shape), B, T_mel))
        dec_inp = self._empty(B, T_mel, H)
        energy_pred = self._empty(B, T_mel) if has else None
        energy_bin = self._empty(B, T_mel, dtype=torch.int32) if has and return_bin else None
        self._call("maa_fs2_finish", self._p(pred_inp), self._p(acc), self._p(m2p), self._p(energy), self._p(self._spk("finish", spk, B)),
                   B, T_mel, self._p(dec_inp), self._p(energy_pred), self._p(energy_bin))
        return (dec_inp, energy_pred, energy_bin) if return_bin else (dec_inp, energy_pred)


def fs2_pitch_config(cfg):
    """maa_fs2_pitch_config of a FastSpeech2MIDI hparams dict with use_pitch_embed (config.FASTSPEECH2_MIDI_CASCADE); refuses what
    the library does not build, with the reason, before any device is touched."""
    what = "FastSpeech2MIDI pitch branch"
    ptype = cfg.get("pitch_type", "frame")
    if ptype == "ph":
        raise L.MaaError("%s: pitch_type 'ph' is not supported: only 'frame' is built (the phoneme-level predictor reads "
                         "encoder_out and gathers the coarse pitch by mel2ph; no shipped singing configuration sets it)" % what)
    if ptype == "cwt":
        raise L.MaaError("%s: pitch_type 'cwt' is not supported: the reference's own modules/fastspeech/fs2.py:191-203 reads "
                         "self.cwt_predictor / self.cwt_stats_layers, which that class never creates, so no oracle exists" % what)
    if ptype != "frame":
        raise L.MaaError("%s: pitch_type %r: the reference has 'frame', 'ph' and 'cwt'" % (what, ptype))
    if cfg.get("pitch_ar", False):
        raise L.MaaError("%s: pitch_ar is not supported: no shipped singing configuration sets it and the autoregressive "
                         "predictor is not built" % what)
    if cfg.get("use_energy_embed", False):
        raise L.MaaError("%s: use_energy_embed is not supported: no shipped configuration sets it and its branch is not built" % what)
    for k in ("use_spk_id", "use_spk_embed"):
        if cfg.get(k, False):
            raise L.MaaError("%s: %s is not supported: the speaker embedding added to pitch_inp and decoder_inp is not built" % (what, k))
    pad = cfg.get("ffn_padding", "SAME")
    if pad != "SAME":
        raise L.MaaError("%s: ffn_padding %r is not supported: only 'SAME' (kernel // 2 zeros on both sides) is built, the causal "
                         "'LEFT' padding (kernel - 1, 0) is not" % (what, pad))
    norm = cfg.get("pitch_norm", "log")
    if norm not in ("log", "standard"):
        raise L.MaaError("%s: pitch_norm %r: the reference has 'log' and 'standard'" % (what, norm))
    c = L.maa_fs2_pitch_config()
    c.hidden_size, c.predictor_hidden = int(cfg["hidden_size"]), int(cfg.get("predictor_hidden", -1))
    c.predictor_layers, c.predictor_kernel = int(cfg.get("predictor_layers", 5)), int(cfg.get("predictor_kernel", 5))
    c.ffn_padding_same = c.pitch_type_frame = 1
    c.pitch_ar = 0
    c.use_uv = int(bool(cfg.get("use_uv", True)))
    c.pitch_norm = 0 if norm == "log" else 1
    c.f0_mean, c.f0_std = float(cfg.get("f0_mean", 0.0)), float(cfg.get("f0_std", 1.0))
    return c


class FS2Pitch(_Handle):
    """maa_fs2_pitch handle: FastSpeech2.add_pitch, pitch_type 'frame' (NeuralSeq/modules/fastspeech/fs2.py:174-220), with the mask
    of :132: PitchPredictor, denorm_f0, f0_to_coarse and the pitch_embed row added to decoder_inp.  state_dict: the pitch_embed /
    pitch_predictor keys (others are ignored)."""

    _destroy = "maa_fs2_pitch_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = dict(cfg)
        self._create(ctx, "maa_fs2_pitch_create", C.byref(fs2_pitch_config(self.cfg)), state_dict=state_dict)

    def forward(self, origin, mel2ph, f0=None, uv=None, return_coarse=False, pred_inp=None):
        """origin [B, T_mel, H] (FastSpeech2MIDI.decode's decoder_inp: 0 where mel2ph is 0), mel2ph [B, T_mel], f0 / uv [B, T_mel]
        or None each (the caller's normalised f0 and unvoiced flags; neither is written) -> (decoder_inp [B, T_mel, H], pitch_pred
        [B, T_mel, 2], f0_denorm [B, T_mel]) on the device; with return_coarse also coarse int32 [B, T_mel], the pitch_embed rows.
        pred_inp [B, T_mel, H]: the predictor's input where it is not origin (a model with speakers: (origin + spk_f0) * tgt)."""
        dev = self.ctx.device
        x = _f32(origin, dev)
        m2p = torch.as_tensor(mel2ph).to(device=dev, dtype=torch.int32).contiguous()
        if x.dim() != 3 or x.shape[2] != self.cfg["hidden_size"] or x.shape[0] < 1 or x.shape[1] < 1:
            raise L.MaaError("FS2Pitch.forward: origin %s is not [B, T_mel, %d]" % (tuple(x.shape), self.cfg["hidden_size"]))
        B, T_mel, H = x.shape
        if tuple(m2p.shape) != (B, T_mel):
            raise L.MaaError("FS2Pitch.forward: mel2ph %s is not [%d, %d]" % (tuple(m2p.shape), B, T_mel))
        f0 = _f32(torch.as_tensor(f0), dev) if f0 is not None else None
        uv = _f32(torch.as_tensor(uv), dev) if uv is not None else None
        for name, t in (("f0", f0), ("uv", uv)):
            if t is not None and tuple(t.shape) != (B, T_mel):
                raise L.MaaError("FS2Pitch.forward: %s %s is not [%d, %d]" % (name, tuple(t.shape), B, T_mel))
        dec_inp = self._empty(B, T_mel, H)
        pitch_pred = self._empty(B, T_mel, 2)
        f0_denorm = self._empty(B, T_mel)
        coarse = self._empty(B, T_mel, dtype=torch.int32) if return_coarse else None
        p = FastSpeech2MIDI._p
        if pred_inp is not None:
            pi = _f32(pred_inp, dev)
            if tuple(pi.shape) != (B, T_mel, H):
                raise L.MaaError("FS2Pitch.forward: pred_inp %s is not origin's [%d, %d, %d]" % (tuple(pi.shape), B, T_mel, H))
            self._call("maa_fs2_pitch_forward_from", p(pi), p(x), p(m2p), p(f0), p(uv), B, T_mel, p(dec_inp), p(pitch_pred),
                       p(f0_denorm), p(coarse))
        else:
            self._call("maa_fs2_pitch_forward", p(x), p(m2p), p(f0), p(uv), B, T_mel, p(dec_inp), p(pitch_pred), p(f0_denorm),
                       p(coarse))
        return (dec_inp, pitch_pred, f0_denorm, coarse) if return_coarse else (dec_inp, pitch_pred, f0_denorm)

    __call__ = forward


class Encoder(_Handle):
    """maa_encoder handle: a conditioning tower on the device.

    kind "text":  BertModel(input_ids) + CLAP Projection per token, FrozenCLAPEmbedder.encode
                  (ldm/modules/encoders/modules.py:204-211, CLAP/clap.py:8-20)
    kind "image": open_clip VisionTransformer + L2 normalisation, FrozenGlobalNormOpenCLIPEmbedder.forward_img
                  (ldm/modules/encoders/modules.py:340-343)"""

    _destroy = "maa_encoder_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = cfg
        c = L.maa_encoder_config()
        c.kind = {"text": 0, "image": 1, "clip_text": 2}[cfg["kind"]]
        c.layers, c.width, c.heads, c.mlp_dim, c.d_proj = cfg["layers"], cfg["width"], cfg["heads"], cfg["mlp_dim"], cfg["d_proj"]
        c.vocab, c.max_positions = cfg.get("vocab", 0), cfg.get("max_positions", 0)
        c.patch, c.image = cfg.get("patch", 0), cfg.get("image", 0)
        c.ln_eps = cfg["ln_eps"]
        self._create(ctx, "maa_encoder_create", C.byref(c), state_dict=state_dict)

    def encode_tokens(self, input_ids):
        """input_ids [B, L] (any integer dtype) -> [B, L, d_proj] (kind "text") / unit-length [B, d_proj] ("clip_text")."""
        if self.cfg["kind"] == "image":
            raise L.MaaError("encode_tokens on an image tower")
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.shape[1] > self.cfg["max_positions"]:
            raise L.MaaError("encode_tokens: input_ids %s must be [B, L <= %d]" % (tuple(ids.shape), self.cfg["max_positions"]))
        ids = ids.to(device=self.ctx.device, dtype=torch.int32).contiguous()
        B, Ln = ids.shape
        shape = (B, Ln, self.cfg["d_proj"]) if self.cfg["kind"] == "text" else (B, self.cfg["d_proj"])
        out = self._empty(*shape, dtype=torch.float32)
        self._call("maa_encoder_text", C.c_void_p(ids.data_ptr()), B, Ln, L.dptr(out))
        return out

    def encode_cls(self, input_ids):
        """The scorer's text side (wav_evaluation/models/clap.py:49-53 + CLAPWrapper.py:177-182): unpadded input_ids
        [B, L] -> Projection of the [CLS] row, unit length, [B, d_proj]."""
        if self.cfg["kind"] != "text":
            raise L.MaaError("encode_cls is the CLAP (BERT) tower's")
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.shape[1] > self.cfg["max_positions"]:
            raise L.MaaError("encode_cls: input_ids %s must be [B, L <= %d]" % (tuple(ids.shape), self.cfg["max_positions"]))
        ids = ids.to(device=self.ctx.device, dtype=torch.int32).contiguous()
        out = self._empty(ids.shape[0], self.cfg["d_proj"], dtype=torch.float32)
        self._call("maa_encoder_text_cls", C.c_void_p(ids.data_ptr()), ids.shape[0], ids.shape[1], L.dptr(out))
        return out

    def encode_image(self, image):
        """image [B, 3, S, S] (preprocessed) -> [B, d_proj], rows of unit length."""
        if self.cfg["kind"] != "image":
            raise L.MaaError("encode_image on a text tower")
        x = _f32(image, self.ctx.device)
        S = self.cfg["image"]
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S):
            raise L.MaaError("encode_image: image %s must be [B, 3, %d, %d]" % (tuple(x.shape), S, S))
        out = self._empty(x.shape[0], self.cfg["d_proj"], dtype=torch.float32)
        self._call("maa_encoder_image", L.dptr(x), x.shape[0], L.dptr(out))
        return out


class ClapAudio(_Handle):
    """maa_clap_audio handle: Cnn14 from the log-mel on + Projection, unit-length rows (the audio side of the CLAP
    best-of-n scorer: wav_evaluation/models/audio.py:150-176, clap.py:8-39, CLAPWrapper.py:184-189)."""

    _destroy = "maa_clap_audio_destroy"

    def __init__(self, ctx, cfg, state_dict):
        self.cfg = cfg
        c = L.maa_clap_audio_config()
        c.mel_bins, c.out_emb, c.d_proj, c.bn_eps = cfg["mel_bins"], cfg["out_emb"], cfg["d_proj"], cfg.get("bn_eps", 1e-5)
        c.n_blocks = _fill(c.channels, cfg["channels"])
        self._create(ctx, "maa_clap_audio_create", C.byref(c),
                     state_dict={k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")})

    def embed(self, logmel, return_embedding=False):
        """logmel [B, 1, T, mel_bins] -> z [B, d_proj] (unit length) [, relu(fc1) embedding [B, out_emb]]."""
        x = _f32(logmel, self.ctx.device)
        if x.dim() != 4 or x.shape[1] != 1 or x.shape[3] != self.cfg["mel_bins"]:
            raise L.MaaError("ClapAudio.embed: logmel %s must be [B, 1, T, %d]" % (tuple(x.shape), self.cfg["mel_bins"]))
        B, _, T, _ = x.shape
        z = self._empty(B, self.cfg["d_proj"], dtype=torch.float32)
        emb = self._empty(B, self.cfg["out_emb"], dtype=torch.float32) if return_embedding else None
        self._call("maa_clap_audio_embed", L.dptr(x), B, T, L.dptr(emb) if emb is not None else None, L.dptr(z))
        return (z, emb) if return_embedding else z


def clap_similarity(ctx, audio_embeddings, text_embeddings, scale=1.0):
    """CLAPWrapper.compute_similarity (CLAPWrapper.py:207-215): [Na, D], [Nt, D] -> [Na, Nt] = scale * audio @ text^T."""
    a, t = _f32(audio_embeddings, ctx.device), _f32(text_embeddings, ctx.device)
    if a.dim() != 2 or t.dim() != 2 or a.shape[1] != t.shape[1]:
        raise L.MaaError("clap_similarity: embeddings %s / %s must be [N, D] with one D" % (tuple(a.shape), tuple(t.shape)))
    out = ctx._empty(a.shape[0], t.shape[0], dtype=torch.float32)
    ctx._call("maa_clap_similarity", L.dptr(a), L.dptr(t), a.shape[0], t.shape[0], a.shape[1], float(scale), L.dptr(out))
    return out


class Spectral(_Handle):
    """maa_spectral handle: waveform [B, n] -> log-mel (framed DFT GEMM -> |.|^p -> mel GEMM -> log), exact fp32.
    cfg: n_fft, hop, n_mels, pad_mode ("constant" | "reflect"), power (1 | 2), log_kind ("db" | "transforms_16000"),
    amin, ref, out_layout ("btm" = [B, frames, n_mels] | "bmt" = [B, n_mels, frames]); basis [2 n_freq, n_fft], melw
    [n_mels, n_freq] are host matrices (audiogpt_amd/mel.py builds them)."""

    _destroy = "maa_spectral_destroy"

    def __init__(self, ctx, cfg, basis, melw):
        self.cfg = dict(cfg)
        c = L.maa_spectral_config()
        c.n_fft, c.hop, c.n_freq, c.n_mels = cfg["n_fft"], cfg["hop"], cfg["n_fft"] // 2 + 1, cfg["n_mels"]
        c.pad_mode = {"constant": 0, "reflect": 1}[cfg["pad_mode"]]
        c.power = int(cfg["power"])
        c.log_kind = {"db": 0, "transforms_16000": 1}[cfg["log_kind"]]
        c.amin, c.ref = float(cfg["amin"]), float(cfg.get("ref", 1.0))
        c.out_layout = {"btm": 0, "bmt": 1}[cfg["out_layout"]]
        bt, bp = L.host_f32(torch.as_tensor(basis))
        mt, mp = L.host_f32(torch.as_tensor(melw))
        if tuple(bt.shape) != (2 * c.n_freq, c.n_fft) or tuple(mt.shape) != (c.n_mels, c.n_freq):
            raise L.MaaError("Spectral: basis %s / melw %s do not match the configuration" % (tuple(bt.shape), tuple(mt.shape)))
        self._create(ctx, "maa_spectral_create", C.byref(c), bp, mp)

    def frames(self, n):
        return 1 + n // self.cfg["hop"]

    def forward(self, wav):
        x = _f32(wav, self.ctx.device)
        if x.dim() == 1:
            x = x[None]
        B, n = x.shape
        T, M = self.frames(n), self.cfg["n_mels"]
        out = self._empty((B, T, M) if self.cfg["out_layout"] == "btm" else (B, M, T))
        self._call("maa_spectral_forward", L.dptr(x), B, n, L.dptr(out))
        return out

    __call__ = forward


class Resampler(_Handle):
    """maa_resampler handle: torchaudio.transforms.Resample(orig, new) with its default sinc / Hann kernel bank
    (kernels [new/g, 2 width + orig/g], built on the host by audiogpt_amd/clap.sinc_resample_kernel), exact fp32."""

    _destroy = "maa_resampler_destroy"

    def __init__(self, ctx, orig, new, width, kernels):
        kt, kp = L.host_f32(torch.as_tensor(kernels))
        self.orig, self.new, self.width = int(orig), int(new), int(width)
        if kt.dim() != 2 or kt.shape[0] != self.new or kt.shape[1] != 2 * width + self.orig:
            raise L.MaaError("Resampler: kernel bank %s must be [new, 2 width + orig]" % (tuple(kt.shape),))
        self._create(ctx, "maa_resampler_create", self.orig, self.new, int(width), kt.shape[1], kp)

    def forward(self, wav):
        x = _f32(wav, self.ctx.device)
        if x.dim() == 1:
            x = x[None]
        B, n = x.shape
        out = self._empty(B, -(-self.new * n // self.orig), dtype=torch.float32)
        self._call("maa_resampler_forward", L.dptr(x), B, n, L.dptr(out))
        return out

    __call__ = forward
