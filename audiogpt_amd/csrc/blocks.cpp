#include "blocks.h"

namespace maa {

void conv_into(Ctx& ctx, const T4& x1, const T4* x2, const PackedW& w, const ConvOpt& o, T4& out) {
    IGemm p;
    p.a1 = x1.p;
    p.lda1 = x1.ld ? x1.ld : x1.C;
    p.C1 = x1.C;
    if (x2) {
        MAA_CHECK(x2->B == x1.B && x2->H == x1.H && x2->W == x1.W, "concat sources differ in shape");
        p.a2 = x2->p;
        p.lda2 = x2->ld ? x2->ld : x2->C;
        p.C2 = x2->C;
    }
    p.Hin = x1.H;
    p.Win = x1.W;
    p.Hout = out.H;
    p.Wout = out.W;
    p.KH = o.KH;
    p.KW = o.KW;
    p.sh = p.sw = o.stride;
    p.dh = p.dw = o.dil;
    p.pw = o.pad;
    p.ph = o.pad_h >= 0 ? o.pad_h : (o.KH > 1 ? o.pad : 0);
    p.up = o.up;
    p.a_act = o.a_act;
    p.a_slope = o.a_slope;
    p.b = w.w;
    p.ldb = w.ld;
    p.b_nk = w.nk;
    p.b_split = w.split;
    if (x1.split) {
        MAA_CHECK(!x2, "a split source cannot be concatenated");
        p.a_split = 1;
    }
    p.M = out.B * out.H * out.W;
    p.K = o.KH * o.KW * (p.C1 + p.C2);
    MAA_CHECK(p.K == w.K, "conv weight K mismatch");
    p.N = o.geglu ? w.N : out.C;
    MAA_CHECK(p.N <= w.N, "conv weight N mismatch");
    p.alpha = o.alpha;
    p.bias = w.bias;
    p.rowadd = o.rowadd;
    p.ld_rowadd = o.ld_rowadd;
    p.res = o.res;
    p.ldr = o.ldr ? o.ldr : out.C;
    p.act = o.act;
    p.act_slope = o.act_slope;
    p.out_scale = o.out_scale;
    p.accumulate = o.accumulate;
    p.geglu = o.geglu;
    p.c_split = o.c_split;
    p.c = out.p;
    p.ldc = o.ldc ? o.ldc : out.C;
    p.c2 = o.c2;
    p.ldc2 = o.ldc2 ? o.ldc2 : out.C;
    p.c2_slope = o.c2_slope;
    launch_igemm(ctx, p);
}

void conv1d_same(Ctx& ctx, const T4& x, const PackedW& w, int k, int dil, float leaky, const float* res, float out_scale,
                 int accumulate, T4& out) {
    // narrow stages (C = 32 / 64): input tile staged once in LDS for all taps -- HBM-bound instead of L2-re-read-bound
    if (x.C == out.C && !x.split && x.H == 1 && x.ld == 0 &&
        launch_halo_conv1d(ctx, x.p, x.B, x.W, x.C, w, k, dil, leaky != 0.f ? leaky : 1.f, res, out_scale, accumulate, out.p))
        return;
    ConvOpt o;
    o.KH = 1;
    o.KW = k;
    o.dil = dil;
    o.pad = (k * dil - dil) / 2;
    o.pad_h = 0;
    if (leaky != 0.f) {
        o.a_act = 1;
        o.a_slope = leaky;
    }
    o.res = res;
    o.out_scale = out_scale;
    o.accumulate = accumulate;
    conv_into(ctx, x, nullptr, w, o, out);
}

void mrf_pair(Ctx& ctx, const T4& x, const PackedW& w1, int k1, int d1, float slope1, const PackedW& w2, int k2, int d2,
              float slope2, const float* res, float out_scale, int accumulate, T4& t1, T4& out) {
    // narrow stages (C = 32 / 64): the pair in one launch, xt stays in LDS (halo_conv1d.hip)
    if (!x.split && x.ld == 0 &&
        launch_halo_pair(ctx, x.p, x.B, x.W, x.C, w1, k1, d1, slope1 != 0.f ? slope1 : 1.f, w2, k2, d2,
                         slope2 != 0.f ? slope2 : 1.f, res, out_scale, accumulate, out.p))
        return;
    conv1d_same(ctx, x, w1, k1, d1, slope1, nullptr, 1.f, 0, t1);
    conv1d_same(ctx, t1, w2, k2, d2, slope2, res, out_scale, accumulate, out);
}

void check_convtr_polyphase(int k, int stride) {
    const std::string at = " (kernel " + std::to_string(k) + ", stride " + std::to_string(stride) + ")";
    MAA_CHECK(stride >= 1 && k >= stride, "conv-transpose needs stride >= 1 and kernel >= stride" + at);
    MAA_CHECK(k % stride == 0, "conv-transpose kernel must be a multiple of the stride" + at);
    MAA_CHECK((k - stride) % 2 == 0, "conv-transpose kernel - stride must be even: padding (kernel - stride) / 2 gives length * stride outputs" + at);
    MAA_CHECK((stride - 1 + (k - stride) / 2) / stride <= 1,
              "conv-transpose polyphase carry (stride - 1 + (kernel - stride) / 2) / stride must be 0 or 1" + at);
}

bool conv_up2_into(Ctx& ctx, const T4& x, const PackedW& w4, T4& out) {
    if (!ctx.tune.up2 || !w4.w || w4.phase_rows == 0 || ctx.dtype == 0 || x.split || x.C % 32 != 0 || x.ld != 0) return false;
    MAA_CHECK(out.B == x.B && out.H == 2 * x.H && out.W == 2 * x.W && out.C == w4.N, "conv_up2: output shape");
    const size_t mk = ctx.ws.mark();
    const long long M = x.rows();
    float* xs = ctx.ws.alloc_f((size_t)x.numel());                  // the source as split32 rows (8 MB at the UNet's 5 x 39 level)
    float* planes = ctx.ws.alloc_f((size_t)4 * M * out.C);          // [4 phases][B, H, W, C]
    IGemm p;
    p.a1 = xs;
    p.lda1 = x.C;
    p.C1 = x.C;
    p.a_split = 1;
    p.Hin = p.Hout = x.H;
    p.Win = p.Wout = x.W;
    p.KH = p.KW = 2;
    p.ph = p.pw = 1;
    p.b = w4.w;
    p.ldb = w4.ld;
    p.b_nk = w4.nk;
    p.b_split = w4.split;
    p.M = (int)M;
    p.K = 4 * x.C;
    p.N = out.C;
    p.bias = w4.bias;
    p.c = planes;
    p.ldc = out.C;
    p.ldr = out.C;
    p.ldc2 = out.C;
    p.zeros = ctx.zeros;
    MAA_CHECK(p.K == w4.K, "conv_up2 weight K mismatch");
    if (!ctx.ws.dry) launch_split32_pack(ctx, x.p, M, x.C, xs);
    const bool ok = launch_igemm_pp_up2(ctx, p, w4.Npad, (long long)w4.phase_rows * w4.ld);
    if (ok) launch_pixel_shuffle2(ctx, planes, x.B, x.H, x.W, out.C, out.p);
    ctx.ws.release(mk);
    return ok;
}

void upsample_conv3x3(Ctx& ctx, const T4& x, const PackedW& w, const PackedW& w_up2, T4& out) {
    if (conv_up2_into(ctx, x, w_up2, out)) return;
    ConvOpt o = conv3x3();
    o.up = 1;
    conv_into(ctx, x, nullptr, w, o, out);
}

void linear_into(Ctx& ctx, const float* a, int lda, long long rows, int K, const PackedW& w, const float* res,
                 int ldr, float* out, int ldc, const LinOpt& o) {
    IGemm p;
    p.a1 = a;
    p.lda1 = lda;
    p.C1 = K;
    p.Hout = 1;
    p.Wout = 1;
    p.M = (int)rows;
    p.K = K;
    MAA_CHECK(K == w.K, "linear weight K mismatch");
    p.N = w.N;
    p.b = w.w;
    p.ldb = w.ld;
    p.b_nk = w.nk;
    p.b_split = w.split;
    p.a_split = o.a_split;
    p.bias = w.bias;
    p.res = res;
    p.ldr = ldr;
    p.geglu = o.geglu;
    p.a_act = o.a_act;
    p.c_split = o.c_split;
    p.act = o.act;
    p.c = out;
    p.ldc = ldc;
    launch_igemm(ctx, p);
}

void attention_into(Ctx& ctx, const float* q, int ldq, int hsq, const float* k, int ldk, int hsk, const float* v,
                    int ldv, int hsv, int B, int heads, int dh, int Nq, int Nk, float alpha, float* out, int ldo,
                    int out_split, int causal, const float* key_mask) {
    MAA_CHECK(!causal || Nq == Nk, "causal attention needs Nq == Nk");
    MAA_CHECK(!causal || !key_mask, "attention takes a causal mask or a key mask, not both");
    if (launch_flash_attention(ctx, q, ldq, hsq, k, ldk, hsk, v, ldv, hsv, B, heads, dh, Nq, Nk, alpha, out, ldo,
                               out_split, causal, key_mask))
        return;
    MAA_CHECK(!out_split, "split32 attention output needs the fused kernel");
    const size_t mk = ctx.ws.mark();
    const int ldS = (Nk + 3) / 4 * 4;
    float* S = ctx.ws.alloc_f((size_t)B * heads * Nq * ldS);
    IGemm p;
    p.a1 = q;
    p.lda1 = ldq;
    p.C1 = dh;
    p.M = Nq;
    p.K = dh;
    p.N = Nk;
    p.b = k;
    p.ldb = ldk;
    p.b_nk = 1;
    p.Z = B * heads;
    p.zin = heads;
    p.a_so = (long long)Nq * ldq;
    p.a_si = hsq;
    p.b_so = (long long)Nk * ldk;
    p.b_si = hsk;
    p.c_so = (long long)heads * Nq * ldS;
    p.c_si = (long long)Nq * ldS;
    p.alpha = alpha;
    p.c = S;
    p.ldc = ldS;
    launch_igemm(ctx, p);
    if (key_mask)
        launch_softmax_masked(ctx, S, (long long)B * heads * Nq, Nk, ldS, key_mask, (long long)heads * Nq);
    else
        launch_softmax(ctx, S, (long long)B * heads * Nq, Nk, ldS, causal ? Nq : 0);
    IGemm r;
    r.a1 = S;
    r.lda1 = ldS;
    r.C1 = Nk;
    r.M = Nq;
    r.K = Nk;
    r.N = dh;
    r.b = v;
    r.ldb = ldv;
    r.Z = B * heads;
    r.zin = heads;
    r.a_so = (long long)heads * Nq * ldS;
    r.a_si = (long long)Nq * ldS;
    r.b_so = (long long)Nk * ldv;
    r.b_si = hsv;
    r.c_so = (long long)Nq * ldo;
    r.c_si = dh;
    r.c = out;
    r.ldc = ldo;
    launch_igemm(ctx, r);
    ctx.ws.release(mk);
}

T4 attn_block(Ctx& ctx, const T4& x, const float* ng, const float* nb, float eps, const PackedW& qkv, const PackedW& proj, int heads,
              int hs, int koff, float alpha) {
    const int C = x.C, HW = x.H * x.W;
    const long long M = x.rows();
    T4 out = alloc_t(ctx, x.B, x.H, x.W, C);
    const size_t mk = ctx.ws.mark();
    float* xn = ctx.ws.alloc_f((size_t)M * C);
    const bool sp = split_for_gemm(ctx, C);
    launch_groupnorm(ctx, x.p, C, C, nullptr, 0, 0, x.B, HW, 32, ng, nb, eps, 0, xn, sp);
    float* t = ctx.ws.alloc_f((size_t)M * 3 * C);
    linear_into(ctx, xn, C, M, C, qkv, nullptr, 0, t, 3 * C, LinOpt(sp));
    float* o = ctx.ws.alloc_f((size_t)M * C);
    attention_into(ctx, t, 3 * C, hs, t + koff, 3 * C, hs, t + 2 * koff, 3 * C, hs, x.B, heads, C / heads, HW, HW, alpha, o, C);
    linear_into(ctx, o, C, M, C, proj, x.p, C, out.p, C);
    ctx.ws.release(mk);
    return out;
}

}  // namespace maa
