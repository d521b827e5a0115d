// Latent-diffusion UNet executor (eps-prediction) on channels-last fp32 activations.
//
// Mirrors the graph of (paths relative to text_to_audio/Make_An_Audio in the reference):
//   ldm/modules/diffusionmodules/openaimodel.py:516-744 (ctor + forward), :255-275 ResBlock,
//   :317-324,356-372 AttentionBlock/QKVAttentionLegacy (inpaint), :134-160 Downsample, :91-119 Upsample
//   ldm/modules/diffusionmodules/custom_openaimodel.py:352-354 (I2A: emb += context.squeeze(1))
//   ldm/modules/attention.py:37-64,152-261 (GEGLU FF, CrossAttention, BasicTransformerBlock, SpatialTransformer)
// Differences from a literal translation (same maths, fewer passes over HBM):
//   * no torch.cat for the skip connections: GroupNorm and the 1x1 skip conv read (h | skip) as two sources
//   * all ResBlock `emb_layers` Linear(SiLU(emb)) run as ONE GEMM per forward, sliced per block
//   * to_q/to_k/to_v of self-attention are one GEMM (N = 3*inner); the cross-attention K/V projections of the
//     (step-invariant) context are computed once per `set_context` and reused by every DDIM step
//   * bias, time-embedding add, residual add and GEGLU are igemm epilogues
//   * a guided DDIM step evaluates the model on cat([x] * 2) with cat([uncond, cond]) (ddim.py:177-199): the two halves differ
//     only in the context, so every layer before the first cross-attention (conv_in, the first ResBlock, the first
//     transformer's norm / proj_in / self-attention / to_q) is the same tensor twice -- computed on one half and duplicated
//     where the halves part (CfgShare::Dup; as two lanes the unconditional lane hands them to the conditional one in the step's
//     CfgPrefix, Export / Import; models.h).  Every kernel is batch-invariant, so the result is bit-identical.
// UNet::Impl holds what outlives a forward: the weights, the layer lists, the K/V cache and the context slabs.  What holds for one
// forward only is a Pass on the stack of Impl::forward, and everything under "execution" is a const member that takes it.
#include "models.h"

#include <atomic>
#include <cmath>
#include <cstdlib>

namespace maa {

namespace {

struct ResW {
    int cin = 0, cout = 0, updown = 0;   // 0 none, 1 down (avg-pool), 2 up (nearest)
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
    PackedW conv1, conv2, skip;
    bool has_skip = false;
    int emb_off = 0;
};
struct STBlockW {
    float *ln1g, *ln1b, *ln2g, *ln2b, *ln3g, *ln3b;
    PackedW qkv1, out1, q2, kv2, out2, ff1, ff2;
    int kv_slot = -1;
};
struct STW {
    int ch = 0, heads = 0, dh = 0;
    float *ng = nullptr, *nb = nullptr;
    PackedW proj_in, proj_out;
    std::vector<STBlockW> blocks;
};
struct AttnW {
    int ch = 0, heads = 0;
    float *ng = nullptr, *nb = nullptr;
    PackedW qkv, proj;
};
struct ConvW {
    PackedW w, w_up2;      // w_up2: the four 2x2 phase weights of an Upsample convolution (pack_conv_up2), else empty
    int cin = 0, cout = 0;
};
enum Kind { kConv, kRes, kST, kAttn, kDown, kUp };
struct Layer {
    Kind kind;
    int idx;
};

// One forward: the context it runs on, the ResBlocks' embedding rows, the lane and the guided step's arrangement
struct Pass {
    Ctx& ctx;
    const float* emb_out = nullptr;
    int emb_ld = 0;           // pitch between the samples' rows of emb_out (0: one row for every sample)
    // a forward over samples [batch_off, batch_off + B) of the batch set_context saw (a lane of a CFG step: ddim.cpp); the
    // caller's x / t / out pointers already stand at that sample, the context rows and the K/V caches are offset here
    int batch_off = 0;
    bool lane = false;
    CfgShare mode = CfgShare::None;
    CfgPrefix* prefix = nullptr;      // Export / Import: the step's hand-over
};
// What a SpatialTransformer's layers before the first cross-attention leave for the rest: the block input (proj_out's residual,
// for every output sample), the residual stream after attn1 and attn2's queries
struct StMid {
    const float *xres, *y1, *q;
};
// The sizes and operand forms of a SpatialTransformer's rows for B samples.  Attention outputs and the GEGLU product feed exactly
// one projection each: in the bf16 modes they are written as split32 rows, so to_out / ff.net.2 take the LDS-DMA engine with no
// per-tile conversion (o_sp, g_sp)
struct StRows {
    int B, HW, inner;
    long long M;
    bool sp_in, sp;
    int o_sp, g_sp;
    float scale;
};

}  // namespace

struct UNet::Impl {
    maa_unet_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    std::vector<ResW> res;
    std::vector<STW> st;
    std::vector<AttnW> attn;
    std::vector<ConvW> convs;
    std::vector<std::vector<Layer>> input, output;
    std::vector<Layer> middle;
    PackedW te0, te2, emb_all, out_conv, out_narrow;
    float *out_g = nullptr, *out_b = nullptr;
    int emb_dim = 0, emb_total = 0;
    // cross-attention K/V cache: one [rows, 2*inner] buffer per transformer block
    unsigned long long serial = next_serial();
    static unsigned long long next_serial() {
        static std::atomic<unsigned long long> n{1};
        return n.fetch_add(1);
    }
    std::vector<float*> kv_cache;
    std::vector<int> kv_inner;
    int kv_rows = 0, kv_len = 0, kv_batch = 0;
    size_t kv_cap_rows = 0;
    DevSlab cfg_context;      // [uncond ; cond] rows of a CFG sample() call
    DevSlab tiled_context;    // the context rows once per crop (set_context with rep > 1, add_context_to_emb only)

    // conv_in, then [ResBlock, SpatialTransformer]: the shape the lanes' hand-over (CfgPrefix) is written for (T2A; anything else
    // keeps the whole evaluation per lane)
    bool prefix_ok() const {
        return cfg.use_spatial_transformer && !cfg.add_context_to_emb && input.size() >= 2 && input[0].size() == 1 &&
               input[0][0].kind == kConv && input[1].size() == 2 && input[1][0].kind == kRes && input[1][1].kind == kST &&
               !st[input[1][1].idx].blocks.empty();
    }

    ~Impl() {
        for (float* p : kv_cache)
            if (p) (void)hipFree(p);
    }

    // ---- construction ---------------------------------------------------------------------------
    Layer add_res(const StateDict& sd, const std::string& p, int cin, int cout, int updown) {
        ResW r;
        r.cin = cin;
        r.cout = cout;
        r.updown = updown;
        r.g1 = ws.vec(sd, p + "in_layers.0.weight");
        r.b1 = ws.vec(sd, p + "in_layers.0.bias");
        r.conv1 = ws.pack_conv(sd, p + "in_layers.2.weight", p + "in_layers.2.bias", 3, 3);
        r.g2 = ws.vec(sd, p + "out_layers.0.weight");
        r.b2 = ws.vec(sd, p + "out_layers.0.bias");
        r.conv2 = ws.pack_conv(sd, p + "out_layers.3.weight", p + "out_layers.3.bias", 3, 3);
        r.has_skip = has(sd, p + "skip_connection.weight");
        if (r.has_skip) r.skip = ws.pack_conv(sd, p + "skip_connection.weight", p + "skip_connection.bias", 1, 1);
        MAA_CHECK(r.has_skip == (cin != cout), "skip_connection presence " + p);
        r.emb_off = emb_total;
        emb_total += cout;
        res.push_back(r);
        return {kRes, (int)res.size() - 1};
    }
    Layer add_st(const StateDict& sd, const std::string& p, int ch, int heads, int dh) {
        STW s;
        s.ch = ch;
        s.heads = heads;
        s.dh = dh;
        const int inner = heads * dh;
        s.ng = ws.vec(sd, p + "norm.weight");
        s.nb = ws.vec(sd, p + "norm.bias");
        s.proj_in = ws.pack_conv(sd, p + "proj_in.weight", p + "proj_in.bias", 1, 1);
        s.proj_out = ws.pack_conv(sd, p + "proj_out.weight", p + "proj_out.bias", 1, 1);
        for (int d = 0; d < cfg.transformer_depth; ++d) {
            const std::string t = p + "transformer_blocks." + std::to_string(d) + ".";
            STBlockW b;
            b.ln1g = ws.vec(sd, t + "norm1.weight");
            b.ln1b = ws.vec(sd, t + "norm1.bias");
            b.ln2g = ws.vec(sd, t + "norm2.weight");
            b.ln2b = ws.vec(sd, t + "norm2.bias");
            b.ln3g = ws.vec(sd, t + "norm3.weight");
            b.ln3b = ws.vec(sd, t + "norm3.bias");
            b.qkv1 = ws.pack_concat(sd, {t + "attn1.to_q.weight", t + "attn1.to_k.weight", t + "attn1.to_v.weight"}, {});
            b.out1 = ws.pack_conv(sd, t + "attn1.to_out.0.weight", t + "attn1.to_out.0.bias", 1, 1);
            b.q2 = ws.pack_conv(sd, t + "attn2.to_q.weight", "", 1, 1);
            b.kv2 = ws.pack_concat(sd, {t + "attn2.to_k.weight", t + "attn2.to_v.weight"}, {});
            b.out2 = ws.pack_conv(sd, t + "attn2.to_out.0.weight", t + "attn2.to_out.0.bias", 1, 1);
            b.ff1 = ws.pack_geglu(sd, t + "ff.net.0.proj.weight", t + "ff.net.0.proj.bias");
            b.ff2 = ws.pack_conv(sd, t + "ff.net.2.weight", t + "ff.net.2.bias", 1, 1);
            b.kv_slot = (int)kv_cache.size();
            kv_cache.push_back(nullptr);
            kv_inner.push_back(inner);
            s.blocks.push_back(b);
        }
        st.push_back(s);
        return {kST, (int)st.size() - 1};
    }
    Layer add_attn(const StateDict& sd, const std::string& p, int ch, int heads) {
        AttnW a;
        a.ch = ch;
        a.heads = heads;
        a.ng = ws.vec(sd, p + "norm.weight");
        a.nb = ws.vec(sd, p + "norm.bias");
        a.qkv = ws.pack_conv(sd, p + "qkv.weight", p + "qkv.bias", 1, 1);
        a.proj = ws.pack_conv(sd, p + "proj_out.weight", p + "proj_out.bias", 1, 1);
        attn.push_back(a);
        return {kAttn, (int)attn.size() - 1};
    }
    Layer add_conv(const StateDict& sd, const std::string& p, int cin, int cout, Kind kind) {
        ConvW c;
        c.cin = cin;
        c.cout = cout;
        c.w = ws.pack_conv(sd, p + "weight", p + "bias", 3, 3);
        if (kind == kUp) c.w_up2 = ws.pack_conv_up2(sd, p + "weight", p + "bias");
        convs.push_back(c);
        return {kind, (int)convs.size() - 1};
    }

    void build(const StateDict& sd) {
        const int mc = cfg.model_channels;
        emb_dim = mc * 4;
        std::vector<std::string> emb_w, emb_b;      // every ResBlock's emb_layers Linear, in emb_off order: packed as one GEMM
        auto res_block = [&](const std::string& p, int cin, int cout, int updown) {
            emb_w.push_back(p + "emb_layers.1.weight");
            emb_b.push_back(p + "emb_layers.1.bias");
            return add_res(sd, p, cin, cout, updown);
        };
        int cur_heads = cfg.num_heads;
        auto attn_layer = [&](const std::string& p, int ch) {      // openaimodel.py:534-553 head bookkeeping
            int heads, dh;
            if (cfg.num_head_channels == -1) {
                heads = cur_heads;
                dh = ch / heads;
            } else {
                heads = ch / cfg.num_head_channels;
                cur_heads = heads;
                dh = cfg.num_head_channels;
            }
            if (cfg.legacy) dh = cfg.use_spatial_transformer ? ch / heads : cfg.num_head_channels;
            if (cfg.use_spatial_transformer) return add_st(sd, p, ch, heads, dh);
            return add_attn(sd, p, ch, dh == -1 ? heads : ch / dh);
        };
        te0 = ws.pack_conv(sd, "time_embed.0.weight", "time_embed.0.bias", 1, 1);
        te2 = ws.pack_conv(sd, "time_embed.2.weight", "time_embed.2.bias", 1, 1);
        auto in_attn = [&](int ds) {
            for (int i = 0; i < cfg.n_attention_resolutions; ++i)
                if (cfg.attention_resolutions[i] == ds) return true;
            return false;
        };
        std::vector<int> chans;
        input.push_back({add_conv(sd, "input_blocks.0.0.", cfg.in_channels, mc, kConv)});
        chans.push_back(mc);
        int ch = mc, ds = 1;
        for (int level = 0; level < cfg.n_channel_mult; ++level) {
            const int m = cfg.channel_mult[level];
            for (int i = 0; i < cfg.num_res_blocks; ++i) {
                const std::string p = "input_blocks." + std::to_string(input.size()) + ".";
                std::vector<Layer> blk;
                blk.push_back(res_block(p + "0.", ch, m * mc, 0));
                ch = m * mc;
                if (in_attn(ds)) blk.push_back(attn_layer(p + "1.", ch));
                input.push_back(blk);
                chans.push_back(ch);
            }
            if (level != cfg.n_channel_mult - 1) {
                const std::string p = "input_blocks." + std::to_string(input.size()) + ".0.";
                if (cfg.resblock_updown)
                    input.push_back({res_block(p, ch, ch, 1)});
                else
                    input.push_back({add_conv(sd, p + "op.", ch, ch, kDown)});
                chans.push_back(ch);
                ds *= 2;
            }
        }
        middle.push_back(res_block("middle_block.0.", ch, ch, 0));
        middle.push_back(attn_layer("middle_block.1.", ch));
        middle.push_back(res_block("middle_block.2.", ch, ch, 0));
        for (int level = cfg.n_channel_mult - 1; level >= 0; --level) {
            const int m = cfg.channel_mult[level];
            for (int i = 0; i < cfg.num_res_blocks + 1; ++i) {
                const int ich = chans.back();
                chans.pop_back();
                const std::string p = "output_blocks." + std::to_string(output.size()) + ".";
                std::vector<Layer> blk;
                blk.push_back(res_block(p + "0.", ch + ich, mc * m, 0));
                ch = mc * m;
                int j = 1;
                if (in_attn(ds)) blk.push_back(attn_layer(p + std::to_string(j++) + ".", ch));
                if (level && i == cfg.num_res_blocks) {
                    const std::string q = p + std::to_string(j++) + ".";
                    if (cfg.resblock_updown)
                        blk.push_back(res_block(q, ch, ch, 2));
                    else
                        blk.push_back(add_conv(sd, q + "conv.", ch, ch, kUp));
                    ds /= 2;
                }
                output.push_back(blk);
            }
        }
        out_g = ws.vec(sd, "out.0.weight");
        out_b = ws.vec(sd, "out.0.bias");
        out_conv = ws.pack_conv(sd, "out.2.weight", "out.2.bias", 3, 3);
        out_narrow = ws.pack_narrow3x3(sd, "out.2.weight", "out.2.bias");
        emb_all = ws.pack_concat(sd, emb_w, emb_b);
        MAA_CHECK(emb_all.N == emb_total, "emb_layers packing");
    }

    // ---- execution: const members over the forward's Pass -----------------------------------------
    T4 run_res(const Pass& p, const ResW& r, const T4& x1, const T4* x2) const {
        Ctx& ctx = p.ctx;
        const int B = x1.B, H = x1.H, W = x1.W;
        const int Ho = r.updown == 1 ? H / 2 : (r.updown == 2 ? H * 2 : H);
        const int Wo = r.updown == 1 ? W / 2 : (r.updown == 2 ? W * 2 : W);
        T4 out = alloc_t(ctx, B, Ho, Wo, r.cout);
        const size_t mk = ctx.ws.mark();
        T4 t1 = alloc_t(ctx, B, H, W, r.cin);
        t1.split = r.updown != 1 && split_for_gemm(ctx, r.cin);     // (the avg-pool of a down block reads fp32)
        // a ResBlock that changes the channel count runs a 1x1 skip convolution over the same (h | skip) rows GroupNorm reads:
        // the apply pass also writes them as split32, so that contraction takes the LDS-DMA engine (both operands by DMA; same
        // products in the same order as the register-staged engine it used to run on -- bit-identical)
        T4 xraw;
        if (r.has_skip && r.updown == 0 && split_for_gemm(ctx, r.cin) && r.skip.split) {
            xraw = alloc_t(ctx, B, H, W, r.cin);
            xraw.split = true;
        }
        launch_groupnorm(ctx, x1.p, x1.C, x1.C, x2 ? x2->p : nullptr, x2 ? x2->C : 0, x2 ? x2->C : 0, B, H * W, 32,
                         r.g1, r.b1, 1e-5f, 1, t1.p, t1.split, xraw.p);
        T4 h1 = alloc_t(ctx, B, Ho, Wo, r.cout);
        ConvOpt o1 = conv3x3();
        o1.rowadd = p.emb_out + r.emb_off;
        o1.ld_rowadd = p.emb_ld;
        const float* resid = nullptr;
        if (r.updown == 1) {          // openaimodel.py:212-214,256-261: avg-pool both h and x, then conv
            MAA_CHECK(!x2, "down ResBlock takes one source");
            T4 tp = alloc_t(ctx, B, Ho, Wo, r.cin), xp = alloc_t(ctx, B, Ho, Wo, r.cin);
            launch_avgpool2(ctx, t1.p, B, H, W, r.cin, tp.p);
            launch_avgpool2(ctx, x1.p, B, H, W, r.cin, xp.p);
            conv_into(ctx, tp, nullptr, r.conv1, o1, h1);
            resid = xp.p;
        } else if (r.updown == 2) {   // :209-211: nearest-2x on both; the conv reads t1 through the gather
            MAA_CHECK(!x2, "up ResBlock takes one source");
            T4 xu = alloc_t(ctx, B, Ho, Wo, r.cin);
            launch_upsample2(ctx, x1.p, B, H, W, r.cin, xu.p);
            o1.up = 1;
            conv_into(ctx, t1, nullptr, r.conv1, o1, h1);
            resid = xu.p;
        } else {
            conv_into(ctx, t1, nullptr, r.conv1, o1, h1);
            resid = x1.p;
        }
        T4 t2 = alloc_t(ctx, B, Ho, Wo, r.cout);
        t2.split = split_for_gemm(ctx, r.cout);
        launch_groupnorm(ctx, h1.p, r.cout, r.cout, nullptr, 0, 0, B, Ho * Wo, 32, r.g2, r.b2, 1e-5f, 1, t2.p, t2.split);
        if (r.has_skip) {
            MAA_CHECK(r.updown == 0, "skip conv with up/down");
            T4 sk = alloc_t(ctx, B, H, W, r.cout);
            if (xraw.p)
                conv_into(ctx, xraw, nullptr, r.skip, ConvOpt(), sk);
            else
                conv_into(ctx, x1, x2, r.skip, ConvOpt(), sk);
            resid = sk.p;
        } else {
            MAA_CHECK(!x2, "identity skip needs a single source");
        }
        ConvOpt o2 = conv3x3();
        o2.res = resid;
        conv_into(ctx, t2, nullptr, r.conv2, o2, out);
        ctx.ws.release(mk);
        return out;
    }

    StRows st_rows(const Ctx& ctx, const STW& s, int B, int HW) const {
        const int inner = s.heads * s.dh;
        const bool sp = split_for_gemm(ctx, inner);
        return {B, HW, inner, (long long)B * HW, split_for_gemm(ctx, s.ch), sp, sp && flash_attention_covers(ctx, s.dh) ? 1 : 0,
                split_for_gemm(ctx, 4 * inner) ? 1 : 0, 1.0f / std::sqrt((float)s.dh)};
    }

    // A transformer block up to its cross-attention: x = attn1(norm1(x)) + x (attention.py:212) -> y1, then attn2's queries of
    // norm2(x) (:213) -> q.  ln, o: scratch rows the whole block shares (LayerNorm output, attention output).  y1, q null: allocated
    // here, each where it is first written (after the self-attention, whose own scratch is the workspace's high-water mark)
    void st_block_head(const Pass& p, const STW& s, const STBlockW& b, const StRows& d, const float* y, float* ln, float* o, float*& y1,
                       float*& q) const {
        Ctx& ctx = p.ctx;
        const int inner = d.inner;
        launch_layernorm(ctx, y, d.M, inner, b.ln1g, b.ln1b, 1e-5f, ln, d.sp);
        float* qkv = ctx.ws.alloc_f((size_t)d.M * 3 * inner);
        linear_into(ctx, ln, inner, d.M, inner, b.qkv1, nullptr, 0, qkv, 3 * inner, LinOpt(d.sp));
        attention_into(ctx, qkv, 3 * inner, s.dh, qkv + inner, 3 * inner, s.dh, qkv + 2 * inner, 3 * inner, s.dh, d.B, s.heads, s.dh,
                       d.HW, d.HW, d.scale, o, inner, d.o_sp);
        if (!y1) y1 = ctx.ws.alloc_f((size_t)d.M * inner);
        linear_into(ctx, o, inner, d.M, inner, b.out1, y, inner, y1, inner, LinOpt(d.o_sp));
        launch_layernorm(ctx, y1, d.M, inner, b.ln2g, b.ln2b, 1e-5f, ln, d.sp);
        if (!q) q = ctx.ws.alloc_f((size_t)d.M * inner);
        linear_into(ctx, ln, inner, d.M, inner, b.q2, nullptr, 0, q, inner, LinOpt(d.sp));
    }

    // The block from its cross-attention on: x = attn2(norm2(x), context) + x (:213), x = ff(norm3(x)) + x (:214) -> the block's
    // output.  The last block's output feeds only proj_out: written as split32 as well (bias + residual are applied before the
    // split, in the same epilogue)
    float* st_block_tail(const Pass& p, const STW& s, const STBlockW& b, const StRows& d, const float* y1, const float* q, float* ln,
                         float* o) const {
        Ctx& ctx = p.ctx;
        const int inner = d.inner;
        MAA_CHECK(ctx.ws.dry || (kv_cache[b.kv_slot] && (p.lane ? p.batch_off + d.B <= kv_batch : kv_batch == d.B)),
                  "set_context must precede forward (batch)");
        const float* kv = kv_cache[b.kv_slot] + (size_t)p.batch_off * kv_len * 2 * inner;
        attention_into(ctx, q, inner, s.dh, kv, 2 * inner, s.dh, kv + inner, 2 * inner, s.dh, d.B, s.heads, s.dh, d.HW, kv_len, d.scale,
                       o, inner, d.o_sp);
        float* y2 = ctx.ws.alloc_f((size_t)d.M * inner);
        linear_into(ctx, o, inner, d.M, inner, b.out2, y1, inner, y2, inner, LinOpt(d.o_sp));
        launch_layernorm(ctx, y2, d.M, inner, b.ln3g, b.ln3b, 1e-5f, ln, d.sp);
        float* g = ctx.ws.alloc_f((size_t)d.M * 4 * inner);
        LinOpt geglu(d.sp, d.g_sp);
        geglu.geglu = 1;
        linear_into(ctx, ln, inner, d.M, inner, b.ff1, nullptr, 0, g, 4 * inner, geglu);
        float* y3 = ctx.ws.alloc_f((size_t)d.M * inner);
        const bool last = &b == &s.blocks.back();
        linear_into(ctx, g, 4 * inner, d.M, 4 * inner, b.ff2, y2, inner, y3, inner, LinOpt(d.g_sp, last && d.sp));
        return y3;
    }

    // GroupNorm, proj_in and the first block up to its cross-attention, on x's samples: everything a guided step's halves share.
    // y1, q: where to leave the results (null: the block's own scratch)
    StMid st_prefix(const Pass& p, const STW& s, const T4& x, const StRows& d, float* ln, float* o, float* y1 = nullptr,
                    float* q = nullptr) const {
        Ctx& ctx = p.ctx;
        float* xn = ctx.ws.alloc_f((size_t)d.M * s.ch);
        launch_groupnorm(ctx, x.p, s.ch, s.ch, nullptr, 0, 0, d.B, d.HW, 32, s.ng, s.nb, 1e-6f, 0, xn, d.sp_in);
        float* y = ctx.ws.alloc_f((size_t)d.M * d.inner);
        linear_into(ctx, xn, s.ch, d.M, s.ch, s.proj_in, nullptr, 0, y, d.inner, LinOpt(d.sp_in));
        st_block_head(p, s, s.blocks.front(), d, y, ln, o, y1, q);
        return {x.p, y1, q};
    }

    // The first block from its cross-attention on, the further blocks in full, proj_out + the block input -> out
    void st_rest(const Pass& p, const STW& s, const StRows& d, const StMid& m, float* ln, float* o, T4& out) const {
        Ctx& ctx = p.ctx;
        const float* y = st_block_tail(p, s, s.blocks.front(), d, m.y1, m.q, ln, o);
        for (size_t i = 1; i < s.blocks.size(); ++i) {
            const size_t n = (size_t)d.M * d.inner;
            float *ln_i = ctx.ws.alloc_f(n), *o_i = ctx.ws.alloc_f(n), *y1 = nullptr, *q = nullptr;
            st_block_head(p, s, s.blocks[i], d, y, ln_i, o_i, y1, q);
            y = st_block_tail(p, s, s.blocks[i], d, y1, q, ln_i, o_i);
        }
        linear_into(ctx, y, d.inner, d.M, d.inner, s.proj_out, m.xres, s.ch, out.p, s.ch, LinOpt(d.sp));
    }

    // A SpatialTransformer under one of the four arrangements of a guided step (models.h CfgShare).  Dup: x holds ONE half of the
    // batch (both halves are equal up to here) and the output has 2 x.B samples; Import: x is the Export lane's block input.
    // What the Export lane publishes (hs0 in forward_body; xres, y1, q here) must be allocated outside every mark / release
    // scope that closes before that lane's forward returns: the other lane reads it until the step's join, which is also what
    // orders the next step's writes behind those reads.
    T4 run_st(const Pass& p, const STW& s, const T4& x, CfgShare mode) const {
        MAA_CHECK(!s.blocks.empty(), "SpatialTransformer without a transformer block");
        Ctx& ctx = p.ctx;
        const StRows in = st_rows(ctx, s, x.B, x.H * x.W), full = st_rows(ctx, s, mode == CfgShare::Dup ? 2 * x.B : x.B, in.HW);
        const size_t n_in = (size_t)in.M * in.inner, n_full = (size_t)full.M * in.inner;
        T4 out = alloc_t(ctx, full.B, x.H, x.W, s.ch);
        float *y1 = nullptr, *q = nullptr;
        if (mode == CfgShare::Export) y1 = ctx.ws.alloc_f(n_in), q = ctx.ws.alloc_f(n_in);
        const size_t mk = ctx.ws.mark();
        float *ln = ctx.ws.alloc_f(n_full), *o = ctx.ws.alloc_f(n_full);
        StMid m;
        switch (mode) {
            case CfgShare::None:
                m = st_prefix(p, s, x, in, ln, o);
                break;
            case CfgShare::Dup: {      // the halves part here: the same block input, queries and residual stream meet two contexts
                float* xd = ctx.ws.alloc_f((size_t)full.M * s.ch);
                launch_dup_half(ctx, x.p, in.M * s.ch, xd);
                m = st_prefix(p, s, x, in, ln, o);
                float *qd = ctx.ws.alloc_f(n_full), *yd = ctx.ws.alloc_f(n_full);
                launch_dup_half(ctx, m.q, (long long)n_in, qd);
                launch_dup_half(ctx, m.y1, (long long)n_in, yd);
                m = {xd, yd, qd};
                break;
            }
            case CfgShare::Export:
                m = st_prefix(p, s, x, in, ln, o, y1, q);
                p.prefix->xres = m.xres, p.prefix->y1 = m.y1, p.prefix->q = m.q;
                p.prefix->filled = true;
                if (!ctx.ws.dry) MAA_HIP(hipEventRecord(p.prefix->ready, ctx.stream));
                break;
            case CfgShare::Import:      // the other lane computed this far on the same x: read in place
                m = {x.p, p.prefix->y1, p.prefix->q};
                break;
        }
        st_rest(p, s, full, m, ln, o, out);
        ctx.ws.release(mk);
        return out;
    }

    T4 run_attn(const Pass& p, const AttnW& a, const T4& x) const {
        // openaimodel.py:317-324 + QKVAttentionLegacy :356-372: per head h the qkv channels are
        // [q_h | k_h | v_h]; q and k are each scaled by ch^-1/4
        const int dh = a.ch / a.heads;
        const float sc = 1.0f / std::sqrt(std::sqrt((float)dh));
        return attn_block(p.ctx, x, a.ng, a.nb, 1e-5f, a.qkv, a.proj, a.heads, 3 * dh, dh, sc * sc);
    }

    // part (in / out): the arrangement the next SpatialTransformer runs under; it parts the halves, so it leaves None behind
    T4 run_layers(const Pass& p, const std::vector<Layer>& layers, T4 h, const T4* skip, CfgShare* part = nullptr) const {
        Ctx& ctx = p.ctx;
        bool first = true;
        for (const Layer& l : layers) {
            const T4* x2 = first ? skip : nullptr;
            switch (l.kind) {
                case kConv:
                case kDown: {   // Downsample: conv3x3 stride 2 pad 1 (openaimodel.py:151-153)
                    const int stride = l.kind == kDown ? 2 : 1;
                    T4 o = alloc_t(ctx, h.B, (h.H - 1) / stride + 1, (h.W - 1) / stride + 1, convs[l.idx].cout);
                    conv_into(ctx, h, nullptr, convs[l.idx].w, conv3x3(stride), o);
                    h = o;
                    break;
                }
                case kRes:
                    h = run_res(p, res[l.idx], h, x2);
                    break;
                case kST:
                    h = run_st(p, st[l.idx], h, part ? *part : CfgShare::None);
                    if (part) *part = CfgShare::None;
                    break;
                case kAttn:
                    h = run_attn(p, attn[l.idx], h);
                    break;
                case kUp: {     // Upsample: nearest 2x then conv3x3 (:116-118), the gather reads through the upsample
                    T4 o = alloc_t(ctx, h.B, h.H * 2, h.W * 2, convs[l.idx].cout);
                    upsample_conv3x3(ctx, h, convs[l.idx].w, convs[l.idx].w_up2, o);
                    h = o;
                    break;
                }
            }
            first = false;
        }
        return h;
    }

    // rows = one per timestep: emb_layers(SiLU(time_embed(timestep_embedding(t)))) for every ResBlock (openaimodel.py:725-726,
    // 218-224, 264) -> out [rows, emb_all.Npad].  `add` (I2A: context.squeeze(1), custom_openaimodel.py:352-354) is a residual
    // of the second time_embed Linear.
    void emb_rows(Ctx& ctx, const float* t, int rows, const float* add, float* out) const {
        const int mc = cfg.model_channels;
        float* te = ctx.ws.alloc_f((size_t)rows * mc);
        launch_timestep_embedding(ctx, t, rows, mc, te);
        float* e1 = ctx.ws.alloc_f((size_t)rows * emb_dim);
        linear_into(ctx, te, mc, rows, mc, te0, nullptr, 0, e1, emb_dim);
        float* emb = ctx.ws.alloc_f((size_t)rows * emb_dim);
        launch_silu(ctx, e1, (long long)rows * emb_dim, e1);
        linear_into(ctx, e1, emb_dim, rows, emb_dim, te2, add, emb_dim, emb, emb_dim);
        float* semb = ctx.ws.alloc_f((size_t)rows * emb_dim);
        launch_silu(ctx, emb, (long long)rows * emb_dim, semb);
        linear_into(ctx, semb, emb_dim, rows, emb_dim, emb_all, nullptr, 0, out, emb_all.Npad);
    }

    // One forward (run twice by run_sized: the dry pass sizes the workspace).  The caller's mode is honoured only with the step's
    // hoisted embedding row, which is what makes the halves of a guided step equal before the first cross-attention: Dup on one
    // stream over an even batch, Export / Import as a lane of a UNet the hand-over is written for (prefix_ok); else None.
    void forward(Ctx& ctx, const float* x_nchw, const float* t, const float* context, int B, int H, int W, float* out_nchw,
                 const UNetForwardOpt& o) const {
        Pass p{ctx};
        p.lane = o.batch_off >= 0;
        p.batch_off = p.lane ? o.batch_off : 0;
        if (context && p.batch_off) context += (size_t)p.batch_off * kv_len * cfg.context_dim;
        const bool handed = o.mode == CfgShare::Export || o.mode == CfgShare::Import;
        MAA_CHECK(!handed || (o.prefix && o.prefix->ready), "guided step: a lane that shares the prefix needs the step's CfgPrefix and its event");
        if (o.emb_row) {
            p.emb_out = o.emb_row;
            if (o.mode == CfgShare::Dup && cfg.use_spatial_transformer && !p.lane && B % 2 == 0) p.mode = CfgShare::Dup;
            if (handed && p.lane && prefix_ok()) p.mode = o.mode, p.prefix = o.prefix;
        } else {
            float* emb_out = ctx.ws.alloc_f((size_t)B * emb_all.Npad);
            emb_rows(ctx, t, B, cfg.add_context_to_emb ? context : nullptr, emb_out);
            p.emb_out = emb_out;
            p.emb_ld = emb_all.Npad;
        }
        if (p.mode == CfgShare::Import)
            forward_rest_of_lane(p, B, H, W, out_nchw);
        else
            forward_body(p, x_nchw, B, H, W, out_nchw);
    }

    void forward_body(const Pass& p, const float* x_nchw, int B, int H, int W, float* out_nchw) const {
        Ctx& ctx = p.ctx;
        if (p.mode == CfgShare::Export) {
            p.prefix->B = B, p.prefix->H = H, p.prefix->W = W;
            p.prefix->filled = false;
        }
        // Dup: samples [B/2, B) repeat samples [0, B/2) (x and the embedding row); only the context rows differ, and the context
        // enters at the first cross-attention -- until then one half is computed and the skip tensors are written twice
        CfgShare part = p.mode;      // None once the halves have parted
        auto both = [&](const T4& t) {
            T4 d = alloc_t(ctx, 2 * t.B, t.H, t.W, t.C);
            launch_dup_half(ctx, t.p, (long long)t.B * t.H * t.W * t.C, d.p);
            return d;
        };
        T4 h = alloc_t(ctx, part == CfgShare::Dup ? B / 2 : B, H, W, cfg.in_channels);
        launch_nchw_to_nhwc(ctx, x_nchw, h.B, cfg.in_channels, H * W, h.p);
        std::vector<T4> hs;
        for (auto& blk : input) {
            h = run_layers(p, blk, h, nullptr, &part);
            hs.push_back(part == CfgShare::Dup ? both(h) : h);
            if (p.mode == CfgShare::Export && hs.size() == 1) p.prefix->hs0 = h.p;      // conv_in's output: the other lane's first skip tensor
        }
        if (part == CfgShare::Dup) h = both(h);      // (no transformer on the way down: the halves part at the middle block at the latest)
        finish(p, h, hs, B, H, W, out_nchw);
    }

    // The conditional lane of a guided step (Import): conv_in, the first ResBlock and the first transformer up to attn2's
    // queries are the unconditional lane's -- same x, same embedding row -- and are read from its workspace.
    void forward_rest_of_lane(const Pass& p, int B, int H, int W, float* out_nchw) const {
        Ctx& ctx = p.ctx;
        const CfgPrefix& f = *p.prefix;
        MAA_CHECK(f.filled && f.B == B && f.H == H && f.W == W, "guided step: the lanes disagree on the shared prefix");
        if (!ctx.ws.dry) MAA_HIP(hipStreamWaitEvent(ctx.stream, f.ready, 0));
        const STW& s0 = st[input[1][1].idx];
        std::vector<T4> hs;
        hs.push_back(view_t(const_cast<float*>(f.hs0), B, H, W, cfg.model_channels));
        T4 h = run_st(p, s0, view_t(const_cast<float*>(f.xres), B, H, W, s0.ch), CfgShare::Import);
        hs.push_back(h);
        for (size_t i = 2; i < input.size(); ++i) {
            h = run_layers(p, input[i], h, nullptr);
            hs.push_back(h);
        }
        finish(p, h, hs, B, H, W, out_nchw);
    }

    // middle block, the way up with the skip tensors, the output head
    void finish(const Pass& p, T4 h, std::vector<T4>& hs, int B, int H, int W, float* out_nchw) const {
        Ctx& ctx = p.ctx;
        const int mc = cfg.model_channels;
        h = run_layers(p, middle, h, nullptr);
        for (auto& blk : output) {
            T4 skip = hs.back();
            hs.pop_back();
            h = run_layers(p, blk, h, &skip);
        }
        T4 hn = alloc_t(ctx, B, H, W, mc);
        hn.split = split_for_gemm(ctx, mc);
        launch_groupnorm(ctx, h.p, mc, mc, nullptr, 0, 0, B, H * W, 32, out_g, out_b, 1e-5f, 1, hn.p, hn.split);
        if (hn.split && ctx.tune.up2 &&
            launch_narrow_conv3x3(ctx, hn.p, mc, B, H, W, mc, out_narrow.w, out_narrow.bias, cfg.out_channels, out_nchw))
            return;      // (bf16x3: the 320 -> 4 convolution on its own kernel, straight to NCHW)
        T4 o = alloc_t(ctx, B, H, W, cfg.out_channels);
        conv_into(ctx, hn, nullptr, out_conv, conv3x3(), o);
        launch_nhwc_to_nchw(ctx, o.p, B, cfg.out_channels, H * W, out_nchw, cfg.out_channels);
    }
};

UNet::UNet(const maa_unet_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    impl_->cfg = cfg;
    impl_->build(sd);
}
UNet::~UNet() = default;
const maa_unet_config& UNet::config() const { return impl_->cfg; }
size_t UNet::weight_bytes() const { return impl_->ws.bytes(); }

void UNet::set_context(Ctx& ctx, const float* context, int B, int L, int rep) {
    Impl& m = *impl_;
    MAA_CHECK(rep >= 1, "set_context: rep must be at least 1");
    if (!m.cfg.use_spatial_transformer) return;
    PrecisionGuard pg(ctx, m.precision);
    // rep > 1 (split_input_params: every sample is evaluated as `rep` crops that share its conditioning): the projections are
    // computed once, for the B samples, behind the cache's B * rep sample slots and copied into them rep times each
    const size_t served = (size_t)B * rep * L, rows = rep > 1 ? served + (size_t)B * L : served;
    if (rows > m.kv_cap_rows) {
        MAA_HIP(hipStreamSynchronize(ctx.stream));      // the old caches may still be read by queued launches
        for (size_t i = 0; i < m.kv_cache.size(); ++i) {
            if (m.kv_cache[i]) MAA_HIP(hipFree(m.kv_cache[i]));
            m.kv_cache[i] = nullptr;
            void* d = nullptr;
            MAA_HIP(hipMalloc(&d, rows * 2 * m.kv_inner[i] * sizeof(float)));
            m.kv_cache[i] = static_cast<float*>(d);
        }
        m.kv_cap_rows = rows;
    }
    for (const STW& s : m.st)
        for (const STBlockW& b : s.blocks) {
            const size_t w = (size_t)2 * s.heads * s.dh;
            float* kv = m.kv_cache[b.kv_slot] + (rep > 1 ? served * w : 0);
            linear_into(ctx, context, m.cfg.context_dim, (long long)B * L, m.cfg.context_dim, b.kv2, nullptr, 0, kv, (int)w);
            if (rep > 1) launch_repeat_rows(ctx, kv, B, (long long)L * w, rep, m.kv_cache[b.kv_slot]);
        }
    m.kv_batch = B * rep;
    m.kv_len = L;
    context_ptr = context;
    if (rep > 1 && m.cfg.add_context_to_emb) {      // (I2A: the time embedding reads the sample's context row as well)
        const long long len = (long long)L * m.cfg.context_dim;
        float* tiled = static_cast<float*>(m.tiled_context.get((size_t)B * rep * len * sizeof(float), ctx.stream));
        launch_repeat_rows(ctx, context, B, len, rep, tiled);
        context_ptr = tiled;
    }
}
int UNet::context_len() const { return impl_->kv_len; }

void UNet::graph_key(std::vector<unsigned long long>& key) const {
    const Impl& m = *impl_;
    key.push_back((unsigned long long)reinterpret_cast<uintptr_t>(this));
    key.push_back(m.serial);                 // (a later UNet may be constructed at a freed one's address)
    key.push_back((unsigned long long)reinterpret_cast<uintptr_t>(context_ptr));
    key.push_back((unsigned long long)m.kv_batch);
    key.push_back((unsigned long long)m.kv_len);
    for (const float* p : m.kv_cache) key.push_back((unsigned long long)reinterpret_cast<uintptr_t>(p));
}

void UNet::set_context_cfg(Ctx& ctx, const float* d_uncond, const float* d_cond, int B, int L, int rep) {
    Impl& m = *impl_;
    const size_t half = (size_t)B * L * m.cfg.context_dim * sizeof(float);
    char* buf = static_cast<char*>(m.cfg_context.get(2 * half, ctx.stream));
    MAA_HIP(hipMemcpyAsync(buf, d_uncond, half, hipMemcpyDeviceToDevice, ctx.stream));
    MAA_HIP(hipMemcpyAsync(buf + half, d_cond, half, hipMemcpyDeviceToDevice, ctx.stream));
    set_context(ctx, reinterpret_cast<const float*>(buf), 2 * B, L, rep);
}

void UNet::forward(Ctx& ctx, const float* x_nchw, const float* t, const float* context, int B, int H, int W, float* out_nchw,
                   const UNetForwardOpt& opt) {
    const Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    run_sized(ctx, [&] { m.forward(ctx, x_nchw, t, context, B, H, W, out_nchw, opt); });
}
int UNet::emb_width() const { return impl_->emb_all.Npad; }
void UNet::emb_table(Ctx& ctx, const float* d_t, int rows, float* d_out) {
    Impl& m = *impl_;
    MAA_CHECK(!m.cfg.add_context_to_emb, "emb_table: this UNet's embedding depends on the sample's context");
    PrecisionGuard pg(ctx, m.precision);
    run_sized(ctx, [&] { m.emb_rows(ctx, d_t, rows, nullptr, d_out); });
}

}  // namespace maa
