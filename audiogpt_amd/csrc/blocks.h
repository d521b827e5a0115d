// Building blocks shared by the UNet, the VAE and the vocoders: thin wrappers that turn a layer into
// igemm / norm launches on channels-last tensors.
#pragma once
#include "maa_internal.h"

namespace maa {

struct T4 {              // dense channels-last activation [B, H, W, C] (sequences: H = 1)
    float* p = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    bool split = false;  // true: rows are split32 lines ([32 bf16 hi | 32 bf16 lo] per 32 channels) instead of fp32
    int ld = 0;          // row pitch in floats; 0 = dense (C)
    long long numel() const { return (long long)B * H * W * C; }
    long long rows() const { return (long long)B * H * W; }
};

inline T4 view_t(float* p, int B, int H, int W, int C) {      // [B, H, W, C] at p
    T4 t;
    t.p = p;
    t.B = B;
    t.H = H;
    t.W = W;
    t.C = C;
    return t;
}
inline T4 alloc_t(Ctx& ctx, int B, int H, int W, int C) {
    return view_t(ctx.ws.alloc_f((size_t)B * H * W * C), B, H, W, C);
}

struct ConvOpt {
    int KH = 1, KW = 1, stride = 1, pad = 0, dil = 1;   // square/isotropic for 2-D; 1-D uses KW only
    int pad_h = -1;                                      // override (VAE downsample pads right/bottom only)
    int up = 0;
    int a_act = 0;
    float a_slope = 0.f;
    const float* rowadd = nullptr;
    int ld_rowadd = 0;
    const float* res = nullptr;   // dense residual with the output's shape
    int act = 0;                  // IGemm::act (4 = leaky-relu with act_slope)
    float act_slope = 0.f;
    float out_scale = 1.f;
    int accumulate = 0;
    int geglu = 0;
    int c_split = 0;              // write the output as split32 lines
    float* c2 = nullptr;          // second output: leaky-relu(c2_slope) of the result as split32 lines (output's shape)
    float c2_slope = 1.f;
    float alpha = 1.f;            // IGemm::alpha
    int ldr = 0, ldc = 0, ldc2 = 0;      // row pitches of res / the output / c2 in floats; 0 = dense (the output's C)
};

inline ConvOpt conv3x3(int stride = 1) {      // the models' 3x3 convolution with padding 1
    ConvOpt o;
    o.KH = o.KW = 3;
    o.pad = 1;
    o.stride = stride;
    return o;
}

// out = conv(x1 ++ x2) with packed weight `w`; output spatial size given by (Ho, Wo)
void conv_into(Ctx& ctx, const T4& x1, const T4* x2, const PackedW& w, const ConvOpt& o, T4& out);
// Dilated "same" Conv1d(C, C, k, dilation = dil) on a sequence [B, 1, L, C] with a leaky-ReLU prologue (leaky = 0: none) and the
// shared epilogue out = (conv + bias + res) * out_scale (+ out): the halo kernel (halo_conv1d.hip) where it accepts the layer,
// else the implicit GEMM.  The vocoders' MRF convolutions and maa_op_mrf_pair go through this one dispatch.
void conv1d_same(Ctx& ctx, const T4& x, const PackedW& w, int k, int dil, float leaky, const float* res, float out_scale,
                 int accumulate, T4& out);
// One ResBlock1 step, out = (c2(leaky(c1(leaky(x, slope1)), slope2)) + res) * out_scale (+ out): the fused pair kernel where it
// accepts the layer, else two conv1d_same calls through the scratch tensor t1 (x's shape).
void mrf_pair(Ctx& ctx, const T4& x, const PackedW& w1, int k1, int d1, float slope1, const PackedW& w2, int k2, int d2,
              float slope2, const float* res, float out_scale, int accumulate, T4& t1, T4& out);
// ConvTranspose1d(k, stride, padding = (k - stride) / 2) as the polyphase GEMMs of WeightStore::pack_convtr_phase: throws on a
// (k, stride) they do not cover -- L * stride output rows and the carry groups 0 and 1 are all that is launched.
void check_convtr_polyphase(int k, int stride);
// Upsample (nearest 2x) + conv3x3 as four 2x2 phase convolutions of the low-resolution source (4 / 9 of the multiplications; bf16
// modes, weights from WeightStore::pack_conv_up2).  false: not applicable here -- the caller runs the 3x3 convolution with ConvOpt::up
bool conv_up2_into(Ctx& ctx, const T4& x, const PackedW& w4, T4& out);
// Upsample + conv3x3 of the UNet and the VAE decoder: the four-phase form, else (exact-fp32 mode, odd channel counts, MAA_PP=off,
// MAA_UP2=0) the 3x3 convolution `w` reading through the virtual-upsample gather
void upsample_conv3x3(Ctx& ctx, const T4& x, const PackedW& w, const PackedW& w_up2, T4& out);
struct LinOpt {
    int geglu = 0;
    int a_act = 0;
    bool a_split = false;         // `a` holds split32 rows (row pitch lda floats)
    int c_split = 0;              // write `out` as split32 rows
    int act = 0;                  // output activation of the igemm epilogue (IGemm::act), applied after bias and residual
    LinOpt() = default;
    explicit LinOpt(bool a_split_, int c_split_ = 0) : a_split(a_split_), c_split(c_split_) {}
};
// linear over rows of a [rows, K] matrix (any leading layout, row pitch lda)
void linear_into(Ctx& ctx, const float* a, int lda, long long rows, int K, const PackedW& w, const float* res,
                 int ldr, float* out, int ldc, const LinOpt& o = LinOpt());

// softmax(alpha * Q K^T) V for `heads` heads of width dh stored head-major inside rows of q/k/v
//   q: [B, Nq, *] pitch ldq;  k, v: [B, Nk, *] pitch ldk / ldv;  per-head column offset = h * head_stride_{q,k,v}
//   out: [B, Nq, heads*dh] dense
void attention_into(Ctx& ctx, const float* q, int ldq, int hsq, const float* k, int ldk, int hsk, const float* v,
                    int ldv, int hsv, int B, int heads, int dh, int Nq, int Nk, float alpha, float* out, int ldo,
                    int out_split = 0, int causal = 0, const float* key_mask = nullptr);
// causal: query i attends to keys 0 .. i only (Nq == Nk)
// key_mask [B, Nk]: a key whose entry is non-zero is hidden from every query of its sample (MultiheadAttention's key_padding_mask,
//   weight exactly 0); a sample with no visible key is written as zeros.  Not together with causal.
// out_split: write split32 rows (only where flash_attention_covers(ctx, dh))
// x + proj(attention(qkv(GroupNorm32(x)))) with q, k, v from one GEMM (N = 3C): `heads` heads of width C / heads, head h's q / k / v
// at columns h * hs + {0, koff, 2 koff} of the qkv rows
T4 attn_block(Ctx& ctx, const T4& x, const float* ng, const float* nb, float eps, const PackedW& qkv, const PackedW& proj, int heads,
              int hs, int koff, float alpha);

// In the bf16 modes a normalisation whose only consumer is a bf16-engine contraction writes bf16 hi/lo planes
// (no per-tile re-splitting of the same activation for every tap and N-tile)
inline bool split_for_gemm(const Ctx& ctx, int C) { return ctx.dtype != 0 && C % 32 == 0; }

// Run a model under its own precision mode (the mode its weights were packed for)
struct PrecisionGuard {
    Ctx& ctx;
    int saved;
    PrecisionGuard(Ctx& c, int mode) : ctx(c), saved(c.dtype) { c.dtype = mode; }
    ~PrecisionGuard() { ctx.dtype = saved; }
};

// Size the workspace with a dry run of `f` (allocations counted, launches skipped), grow the slab if needed
// (never during graph capture: sizes are fixed per shape), then run `f` for real.
template <class F>
void run_sized(Ctx& ctx, F&& f) {
    ctx.ws.reset();
    ctx.ws.dry = true;
    try {
        f();
    } catch (...) {
        ctx.ws.dry = false;
        throw;
    }
    ctx.ws.dry = false;
    const size_t need = ctx.ws.mark_high();
    if (need > ctx.ws.capacity()) ctx.ws.reserve(need + need / 8);
    ctx.ws.reset();
    f();
}

}  // namespace maa
