// The layers DiffSinger's PitchExtractor and FastSpeech2MIDI share on the host (seq_layers.h).
#include "seq_layers.h"

#include "models.h"

#include <cmath>

namespace maa {

void conv1d_act(Ctx& ctx, const float* x, int Cin, const PackedW& w, int k, int B, int T, int act, float alpha, float* y) {
    T4 a = seq_t4(const_cast<float*>(x), B, T, Cin), o = seq_t4(y, B, T, w.N);
    ConvOpt co;
    co.KW = k;
    co.pad = (k - 1) / 2;
    co.pad_h = 0;
    co.act = act;
    co.alpha = alpha;
    conv_into(ctx, a, nullptr, w, co, o);
}

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

void SinusoidTable::build(WeightStore& ws, int init_rows, int dim) {
    rows_ = init_rows, dim_ = dim;
    table_ = ws.upload(sinusoid_table(rows_, dim_));
}

void SinusoidTable::grow(Ctx& ctx, int T) {
    if (T + 1 <= rows_) return;
    host_ = sinusoid_table(T + 1, dim_);
    float* d = static_cast<float*>(big_.get(host_.size() * sizeof(float), ctx.stream));
    MAA_HIP(hipMemcpyAsync(d, host_.data(), host_.size() * sizeof(float), hipMemcpyHostToDevice, ctx.stream));
    table_ = d;
    rows_ = T + 1;
}

void ConvPredictor::build(WeightStore& ws, const StateDict& sd, const std::string& model, const std::string& prefix, int n_layers,
                          int k, int c_in, int c_p, int n_out) {
    kernel = k, Cin = c_in, Cp = c_p;
    for (int i = 0; i < n_layers; ++i) {
        const std::string p = prefix + "conv." + std::to_string(i) + ".";
        conv.push_back(ws.pack_conv(sd, p + "1.weight", p + "1.bias", 1, k));
        MAA_CHECK(conv.back().N == Cp && conv.back().K == k * (i ? Cp : Cin), model + " conv shape " + p);
        MAA_CHECK(get(sd, p + "3.weight").numel() == Cp, model + " LayerNorm shape " + p);
        ln_w.push_back(ws.vec(sd, p + "3.weight"));
        ln_b.push_back(ws.vec(sd, p + "3.bias"));
    }
    MAA_CHECK(get(sd, prefix + "linear.weight").numel() == (long long)n_out * Cp && get(sd, prefix + "linear.bias").numel() == n_out,
              model + " linear must be [" + std::to_string(n_out) + ", C_p]");
    lin_w = ws.vec(sd, prefix + "linear.weight");
    lin_b = ws.vec(sd, prefix + "linear.bias");
}

const float* ConvPredictor::run(Ctx& ctx, const float* x, int B, int T, const float* mask_or_null, float* a, float* b) const {
    const long long rows = (long long)B * T;
    const int n = (int)conv.size();
    for (int i = 0; i < n; ++i) {
        conv1d_act(ctx, i ? b : x, i ? Cp : Cin, conv[i], kernel, B, T, 2, 1.f, a);
        if (i + 1 == n) break;
        launch_layernorm(ctx, a, rows, Cp, ln_w[i], ln_b[i], EPS, b);
        if (mask_or_null) launch_pe_affine_mask(ctx, b, rows, Cp, nullptr, nullptr, mask_or_null, b);
    }
    return a;
}

}  // namespace maa
