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
// The "same" Conv1d + ReLU, the sinusoid table and the predictor stack are seq_layers.h's, shared with fs2.cpp; what stays here
// is the Prenet with its BatchNorm folding, ConvStacks and the order of the whole.
#include "models.h"
#include "seq_layers.h"

#include <cmath>
#include <vector>

namespace maa {

namespace {

constexpr int PE_PRENET_LAYERS = 3, PE_PREDICTOR_LAYERS = 5, PE_KERNEL = 5, PE_TABLE_INIT = 4096;
constexpr float PE_EPS = 1e-5f;

}  // namespace

struct PitchExtractor::Impl {
    maa_pitch_extractor_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    int Cp = 0;                         // predictor width
    std::vector<PackedW> pre_conv, enc_conv;
    std::vector<float*> bn_scale, bn_shift, gn_w, gn_b;
    PackedW pre_out, enc_in, enc_out;
    ConvPredictor pp;
    float alpha = 1.f;
    SinusoidTable table;                // [max(4096, T + 1), hidden_size]

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
        pp.build(ws, sd, "PitchPredictor", "pitch_predictor.", PE_PREDICTOR_LAYERS, cfg.predictor_kernel, H, Cp, 2);
        alpha = get(sd, "pitch_predictor.pos_embed_alpha").data[0];
        // (mel_prenet.layers.i.2.num_batches_tracked and pitch_predictor.embed_positions._float_tensor are bookkeeping: not read)
        table.build(ws, PE_TABLE_INIT, H);
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
            conv1d_act(ctx, src, i ? H : M, pre_conv[i], PE_KERNEL, B, T, 2, 1.f, y);
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
                T4 tx = seq_t4(x, B, T, H), ty = seq_t4(y, B, T, H);
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
        launch_pe_pos_add(ctx, h, B, T, H, table.ptr(), alpha, x);
        const float* y = pp.run(ctx, x, B, T, nullptr, h, x);          // (a LayerNorm writes over x, which its convolution has read)
        launch_pe_head(ctx, y, rows, Cp, pp.gamma(), pp.beta(), pp.EPS, pp.lin_w, pp.lin_b, mask, cfg.pitch_norm, cfg.f0_mean, cfg.f0_std,
                       cfg.use_uv, pitch_pred, f0);
    }
};

PitchExtractor::PitchExtractor(const maa_pitch_extractor_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    impl_->cfg = cfg;
    impl_->Cp = cfg.predictor_hidden > 0 ? cfg.predictor_hidden : cfg.hidden_size;
    impl_->build(sd);
}
PitchExtractor::~PitchExtractor() = default;
const maa_pitch_extractor_config& PitchExtractor::config() const { return impl_->cfg; }

void PitchExtractor::forward(Ctx& ctx, const float* mel, int B, int T, float* pitch_pred, float* f0, float* hidden_out) {
    Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    m.table.grow(ctx, T);
    run_sized(ctx, [&] { m.forward(ctx, mel, B, T, pitch_pred, f0, hidden_out); });
}

}  // namespace maa
