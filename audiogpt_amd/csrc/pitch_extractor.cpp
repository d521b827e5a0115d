// DiffSinger's PitchExtractor on the device: mel [B, T, n_mel_bins] -> pitch_pred [B, T, 2] and f0 [B, T], the network the
// e2e singing configurations run between the diffusion's mel and the NSF vocoder (NeuralSeq/inference/svs/ds_e2e.py:36-45).
//
// Mirrors NeuralSeq/modules/fastspeech/pe.py:7-149 (Prenet, ConvBlock, ConvStacks, PitchExtractor),
// modules/fastspeech/tts_modules.py:217-260 (PitchPredictor) and utils/pitch_utils.py:63-76 (denorm_f0).
// Layout: channels-last rows [B*T, C]; every Conv1d is an implicit GEMM over the rows with zero padding per sample, its ReLU
// the igemm epilogue; the Linears are plain GEMMs.  What lies between the contractions is pitch.hip:
//   * BatchNorm1d (eval) follows the ReLU and precedes the mask and the next layer's zero padding, so it cannot be folded into
//     a convolution: scale = w / sqrt(running_var + eps), shift = b - running_mean * scale, applied with the mask in one pass
//   * GroupNorm's statistics run over all T frames of a sample (padding frames included, as in the reference)
//   * the positions are data-dependent (make_positions on channel 0): counted on the device, no host round trip
//   * the sinusoid table is built on the host with the reference's fp32 formula: init_size rows at creation, grown to T + 1
// forward issues launches on the context's stream only: no device-to-host copy, no synchronisation (growing the workspace
// or the table past 4096 rows, once per new largest shape, reallocates).
#include "models.h"

#include <cmath>
#include <vector>

namespace maa {

void launch_pe_gn_relu_res(Ctx& ctx, const float* y, const float* res, int B, int T, int C, int groups, const float* gamma,
                           const float* beta, float eps, float* out);
void launch_pe_head(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                    const float* w, const float* bias, const float* mask, int norm, float f0_mean, float f0_std, int use_uv,
                    float* pitch_pred, float* f0);

// SinusoidalPositionalEmbedding.get_embedding(rows, dim, padding_idx = 0) in fp32 (common_layers.py:104-121)
std::vector<float> sinusoid_table(int rows, int dim) {
    const int half = dim / 2;
    const float step = (float)-(std::log(10000.0) / (double)(half - 1));
    std::vector<float> freq(half), tab((size_t)rows * dim, 0.f);
    for (int j = 0; j < half; ++j) freq[j] = std::exp((float)j * step);
    for (int p = 1; p < rows; ++p)              // (row 0 = padding_idx stays zero)
        for (int j = 0; j < half; ++j) {
            const float a = (float)p * freq[j];
            tab[(size_t)p * dim + j] = std::sin(a);
            tab[(size_t)p * dim + half + j] = std::cos(a);
        }
    return tab;
}

namespace {

constexpr int PE_PRENET_LAYERS = 3, PE_PREDICTOR_LAYERS = 5, PE_KERNEL = 5, PE_TABLE_INIT = 4096;
constexpr float PE_EPS = 1e-5f;

inline T4 seq(float* p, int B, int T, int C) {
    T4 t;
    t.p = p;
    t.B = B;
    t.H = 1;
    t.W = T;
    t.C = C;
    return t;
}

}  // namespace

struct PitchExtractor::Impl {
    maa_pitch_extractor_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    int Cp = 0;                         // predictor width
    std::vector<PackedW> pre_conv, enc_conv, pp_conv;
    std::vector<float*> bn_scale, bn_shift, gn_w, gn_b, ln_w, ln_b;
    PackedW pre_out, enc_in, enc_out;
    float *lin_w = nullptr, *lin_b = nullptr;
    float alpha = 1.f;
    const float* table = nullptr;       // [table_rows, hidden_size] on the device
    int table_rows = 0;
    DevSlab table_big;                  // the table once T + 1 exceeds init_size
    std::vector<float> table_host;      // source of the grown table's upload

    void build(const StateDict& sd) {
        const int H = cfg.hidden_size;
        for (int i = 0; i < PE_PRENET_LAYERS; ++i) {
            const std::string p = "mel_prenet.layers." + std::to_string(i) + ".";
            pre_conv.push_back(ws.pack_conv(sd, p + "0.weight", p + "0.bias", 1, PE_KERNEL));
            MAA_CHECK(pre_conv.back().N == H && pre_conv.back().K == PE_KERNEL * (i ? H : cfg.n_mel_bins), "Prenet conv shape " + p);
            const HostTensor &w = get(sd, p + "2.weight"), &b = get(sd, p + "2.bias"), &m = get(sd, p + "2.running_mean"),
                             &v = get(sd, p + "2.running_var");
            MAA_CHECK(w.numel() == H && b.numel() == H && m.numel() == H && v.numel() == H, "Prenet BatchNorm shape " + p);
            std::vector<float> sc(H), sh(H);
            for (int c = 0; c < H; ++c) {
                sc[c] = w.data[c] / std::sqrt(v.data[c] + PE_EPS);
                sh[c] = b.data[c] - m.data[c] * sc[c];
            }
            bn_scale.push_back(ws.upload(sc));
            bn_shift.push_back(ws.upload(sh));
        }
        pre_out = ws.pack_conv(sd, "mel_prenet.out_proj.weight", "mel_prenet.out_proj.bias", 1, 1);
        if (cfg.conv_layers > 0) {
            enc_in = ws.pack_conv(sd, "mel_encoder.in_proj.weight", "mel_encoder.in_proj.bias", 1, 1);
            for (int i = 0; i < cfg.conv_layers; ++i) {
                const std::string p = "mel_encoder.conv." + std::to_string(i) + ".";
                enc_conv.push_back(ws.pack_conv(sd, p + "conv.conv.weight", p + "conv.conv.bias", 1, PE_KERNEL));
                MAA_CHECK(get(sd, p + "norm.weight").numel() == H, "ConvStacks GroupNorm shape " + p);
                gn_w.push_back(ws.vec(sd, p + "norm.weight"));
                gn_b.push_back(ws.vec(sd, p + "norm.bias"));
            }
            enc_out = ws.pack_conv(sd, "mel_encoder.out_proj.weight", "mel_encoder.out_proj.bias", 1, 1);
            MAA_CHECK(enc_in.N == H && enc_out.N == H, "ConvStacks projection shape");
        }
        for (int i = 0; i < PE_PREDICTOR_LAYERS; ++i) {
            const std::string p = "pitch_predictor.conv." + std::to_string(i) + ".";
            pp_conv.push_back(ws.pack_conv(sd, p + "1.weight", p + "1.bias", 1, cfg.predictor_kernel));
            MAA_CHECK(pp_conv.back().N == Cp && pp_conv.back().K == cfg.predictor_kernel * (i ? Cp : H), "PitchPredictor conv shape " + p);
            MAA_CHECK(get(sd, p + "3.weight").numel() == Cp, "PitchPredictor LayerNorm shape " + p);
            ln_w.push_back(ws.vec(sd, p + "3.weight"));
            ln_b.push_back(ws.vec(sd, p + "3.bias"));
        }
        const HostTensor& lw = get(sd, "pitch_predictor.linear.weight");
        MAA_CHECK(lw.numel() == 2LL * Cp && get(sd, "pitch_predictor.linear.bias").numel() == 2, "PitchPredictor linear must be [2, C_p]");
        lin_w = ws.vec(sd, "pitch_predictor.linear.weight");
        lin_b = ws.vec(sd, "pitch_predictor.linear.bias");
        alpha = get(sd, "pitch_predictor.pos_embed_alpha").data[0];
        // (mel_prenet.layers.i.2.num_batches_tracked and pitch_predictor.embed_positions._float_tensor are bookkeeping: not read)
        table_rows = PE_TABLE_INIT;
        table = ws.upload(sinusoid_table(table_rows, H));
    }

    // max_pos = padding_idx + 1 + seq_len rows (common_layers.py:126-133): rebuilt and uploaded when T outgrows the table
    void grow_table(Ctx& ctx, int T) {
        if (T + 1 <= table_rows) return;
        table_host = sinusoid_table(T + 1, cfg.hidden_size);
        float* d = static_cast<float*>(table_big.get(table_host.size() * sizeof(float), ctx.stream));
        MAA_HIP(hipMemcpyAsync(d, table_host.data(), table_host.size() * sizeof(float), hipMemcpyHostToDevice, ctx.stream));
        table = d;
        table_rows = T + 1;
    }

    void conv(Ctx& ctx, float* x, int Cin, const PackedW& w, int k, int B, int T, float* y) {
        T4 a = seq(x, B, T, Cin), o = seq(y, B, T, w.N);
        ConvOpt co;
        co.KW = k;
        co.pad = (k - 1) / 2;
        co.pad_h = 0;
        co.act = 2;
        conv_into(ctx, a, nullptr, w, co, o);
    }

    void forward(Ctx& ctx, const float* mel, int B, int T, float* pitch_pred, float* f0, float* hidden_out) {
        const int H = cfg.hidden_size, M = cfg.n_mel_bins;
        const long long rows = (long long)B * T;
        const size_t wide = (size_t)rows * (H > Cp ? H : Cp);
        float* mask = ctx.ws.alloc_f((size_t)rows);
        float* a = ctx.ws.alloc_f(wide);
        float* b = ctx.ws.alloc_f(wide);
        launch_pe_frame_mask(ctx, mel, rows, M, mask);
        // ---- Prenet (pe.py:23-41)
        const float* src = mel;
        for (int i = 0; i < PE_PRENET_LAYERS; ++i) {
            float* y = i % 2 ? b : a;
            conv(ctx, const_cast<float*>(src), i ? H : M, pre_conv[i], PE_KERNEL, B, T, y);
            launch_pe_affine_mask(ctx, y, rows, H, bn_scale[i], bn_shift[i], mask, y);
            src = y;
        }
        float* h = b;                                                     // (the third layer left its output in a)
        linear_into(ctx, src, H, rows, H, pre_out, nullptr, 0, h, H);
        launch_pe_affine_mask(ctx, h, rows, H, nullptr, nullptr, mask, h);
        // ---- ConvStacks (pe.py:98-116)
        if (cfg.conv_layers > 0) {
            float *x = a, *y = b;
            linear_into(ctx, h, H, rows, H, enc_in, nullptr, 0, x, H);
            for (int i = 0; i < cfg.conv_layers; ++i) {
                T4 tx = seq(x, B, T, H), ty = seq(y, B, T, H);
                conv1d_same(ctx, tx, enc_conv[i], PE_KERNEL, 1, 0.f, nullptr, 1.f, 0, ty);
                launch_pe_gn_relu_res(ctx, y, x, B, T, H, H / 16, gn_w[i], gn_b[i], PE_EPS, y);
                float* t = x;
                x = y;
                y = t;
            }
            linear_into(ctx, x, H, rows, H, enc_out, nullptr, 0, y, H);
            h = y;
        }
        if (hidden_out && !ctx.ws.dry)
            MAA_HIP(hipMemcpyAsync(hidden_out, h, (size_t)rows * H * sizeof(float), hipMemcpyDeviceToDevice, ctx.stream));
        // ---- PitchPredictor (tts_modules.py:247-260) and denorm_f0
        float* x = h == a ? b : a;
        launch_pe_pos_add(ctx, h, B, T, H, table, alpha, x);
        float* y = h;
        for (int i = 0; i < PE_PREDICTOR_LAYERS; ++i) {
            conv(ctx, x, i ? Cp : H, pp_conv[i], cfg.predictor_kernel, B, T, y);
            if (i + 1 < PE_PREDICTOR_LAYERS) {
                launch_layernorm(ctx, y, rows, Cp, ln_w[i], ln_b[i], PE_EPS, x);
            } else {
                launch_pe_head(ctx, y, rows, Cp, ln_w[i], ln_b[i], PE_EPS, lin_w, lin_b, mask, cfg.pitch_norm, cfg.f0_mean, cfg.f0_std,
                               cfg.use_uv, pitch_pred, f0);
            }
        }
    }
};

PitchExtractor::PitchExtractor(const maa_pitch_extractor_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    impl_->cfg = cfg;
    impl_->Cp = cfg.predictor_hidden > 0 ? cfg.predictor_hidden : cfg.hidden_size;
    try {
        impl_->build(sd);
    } catch (...) {
        delete impl_;
        throw;
    }
}
PitchExtractor::~PitchExtractor() { delete impl_; }
const maa_pitch_extractor_config& PitchExtractor::config() const { return impl_->cfg; }

void PitchExtractor::forward(Ctx& ctx, const float* mel, int B, int T, float* pitch_pred, float* f0, float* hidden_out) {
    Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    m.grow_table(ctx, T);
    run_sized(ctx, [&] { m.forward(ctx, mel, B, T, pitch_pred, f0, hidden_out); });
}

}  // namespace maa
