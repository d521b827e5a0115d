// Host-side layers that DiffSinger's sequence models share (pitch_extractor.cpp, fs2.cpp): the "same" Conv1d with an epilogue
// activation, the growing sinusoid table, and the convolutional predictor stack.  Activations are channels-last rows [B*T, C].
#pragma once
#include "blocks.h"

namespace maa {

inline T4 seq_t4(float* p, int B, int T, int C) {
    T4 t;
    t.p = p;
    t.B = B;
    t.H = 1;
    t.W = T;
    t.C = C;
    return t;
}

// y [B*T, w.N] = act(alpha * Conv1d(Cin, w.N, k, padding = (k - 1) / 2)(x) + bias), zero padding per sample: an implicit GEMM
// over the rows with the activation (IGemm::act) in its epilogue
void conv1d_act(Ctx& ctx, const float* x, int Cin, const PackedW& w, int k, int B, int T, int act, float alpha, float* y);

// SinusoidalPositionalEmbedding.get_embedding(rows, dim, padding_idx = 0) in fp32 (common_layers.py:104-121)
std::vector<float> sinusoid_table(int rows, int dim);

// That table on the device: init_rows rows uploaded with the weights, rebuilt on the host and uploaded again when a sequence
// outgrows it (max_pos = padding_idx + 1 + seq_len rows, common_layers.py:126-133; once per new largest T, reallocates)
class SinusoidTable {
public:
    void build(WeightStore& ws, int init_rows, int dim);
    void grow(Ctx& ctx, int T);
    const float* ptr() const { return table_; }      // [rows, dim]

private:
    const float* table_ = nullptr;
    int rows_ = 0, dim_ = 0;
    DevSlab big_;                  // the table once T + 1 exceeds init_rows
    std::vector<float> host_;      // source of the grown table's upload
};

// PitchPredictor / DurationPredictor (tts_modules.py:59-143, 217-260): n x (Conv1d "same" -> ReLU -> LayerNorm [-> mask]) and
// Linear(C_p, n_out).  The last LayerNorm and the Linear are one head kernel of the caller's (pitch.hip, fs2.hip), which is
// where the two predictors differ; run() stops after the last convolution.
struct ConvPredictor {
    static constexpr float EPS = 1e-5f;      // of every LayerNorm, the head's included
    std::vector<PackedW> conv;
    std::vector<float*> ln_w, ln_b;
    float *lin_w = nullptr, *lin_b = nullptr;      // [n_out, C_p], [n_out]
    int kernel = 0, Cin = 0, Cp = 0;

    // weights `prefix`conv.i.1 / conv.i.3 / linear of the state dict; `model` names the network in the shape errors
    void build(WeightStore& ws, const StateDict& sd, const std::string& model, const std::string& prefix, int n_layers, int k,
               int c_in, int c_p, int n_out);
    // x [B*T, Cin] -> the last convolution's (ReLU'd) output [B*T, C_p], which is a.  Layer i: conv into a, LayerNorm a -> b,
    // b times mask[row] where a mask is given, and b feeds layer i + 1: b may be x itself
    const float* run(Ctx& ctx, const float* x, int B, int T, const float* mask_or_null, float* a, float* b) const;
    const float* gamma() const { return ln_w.back(); }      // the last layer's LayerNorm, for the head
    const float* beta() const { return ln_b.back(); }
};

}  // namespace maa
