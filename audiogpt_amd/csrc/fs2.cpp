// DiffSinger's FastSpeech2MIDI on the device: tokens + note features -> encoder_out and durations (encode), durations -> mel2ph
// (length_regulate), encoder_out + mel2ph -> decoder_inp and the coarse mel (decode): what DiffSingerE2EInfer.forward_model
// runs before the diffusion (NeuralSeq/inference/svs/ds_e2e.py, modules/diff/shallow_diffusion_tts.py:244-251).
//
// Mirrors NeuralSeq/modules/diffsinger_midi/fs2.py:11-118 (FastspeechMIDIEncoder, FastSpeech2MIDI), modules/fastspeech/fs2.py:22-72,
// 140-163,222-226 (FastSpeech2: add_dur, run_decoder), modules/fastspeech/tts_modules.py:59-143 (DurationPredictor), :179-214
// (LengthRegulator), :276-384 (FFTBlocks, FastspeechEncoder, FastspeechDecoder), modules/commons/common_layers.py:485-587
// (TransformerFFNLayer, EncSALayer) with :165-293 (MultiheadAttention, bias = False) and espnet_positional_embedding.py:14-45,89-113.
// Layout: channels-last rows [B*T, C]; the FFN's Conv1d(H, 4H, k) and the predictor's Conv1d are implicit GEMMs over the rows with
// zero padding per sample, GELU / ReLU their epilogue; in_proj / out_proj / ffn_2 / mel_out are plain GEMMs; the attention is the
// masked kernel at head width 128.  What lies between is fs2.hip and the row kernels shared with the pitch extractor.
//   * ffn_1's `* kernel_size ** -0.5` sits between its bias and the GELU: alpha of the GEMM, with the bias scaled once on the host
//   * a padding row is NOT zero where in_proj and ffn_1 read it: LayerNorm of a zero row is its bias, and through the k-wide
//     convolution that reaches the live neighbours, as in the reference.  Rows are masked where the reference masks them, no earlier
//   * one FFTBlocks serves the encoder (mask = token 0) and the decoder (mask = an all-zero decoder_inp row, found on the device)
// The entry points issue launches on the context's stream only: no device-to-host copy, no synchronisation.  T_mel sizes
// decode's outputs, so the caller reads the B totals between encode and decode -- the one read per utterance.
// The cascade configurations (use_pitch_embed: inference/svs/ds_cascade.py, midi/cascade/opencs/ds60_rel.yaml) add FS2Pitch, a
// second handle: decode without the decoder -> its PitchPredictor and pitch tail finish decoder_inp (fs2.py:125-132,187-220) ->
// run_decoder, decode's second half on that decoder_inp.
// The plain FastSpeech2 (cfg.plain: modules/fastspeech/fs2.py:22-226, the fs2 of every configuration without use_midi) is the same
// handle type: the shared layers above, no note terms, sinusoid rows by token count (or rel_pos), the speaker tables or projection and
// the energy branch; in fs2.py's order: [speaker] -> encode_plain -> length_regulate -> decode without the decoder -> [add_speaker]
// -> [FS2Pitch, its predictor's input apart from origin] -> finish -> run_decoder.
// The "same" Conv1d with its epilogue activation, the decoder's sinusoid table and the predictor stack are seq_layers.h's,
// shared with pitch_extractor.cpp; what stays here is the embeddings, FFTBlocks, the length regulator and the order of the whole.
#include "models.h"
#include "seq_layers.h"

#include <cmath>
#include <vector>

namespace maa {

void launch_fs2_embed(const Ctx& ctx, const int* tok, const int* midi, const float* midi_dur, const int* slur, const float* E, int vocab,
                      const float* Mi, const float* dw, const float* db, const float* S, const float* pe, float scale, int B, int T, int H,
                      float* x, float* nonpad, float* hidden);
void launch_fs2_length(Ctx& ctx, const int* dur, int B, int T, int* totals, int T_mel, int* mel2ph);
void launch_fs2_expand(const Ctx& ctx, const float* enc, const int* mel2ph, int B, int T, int T_mel, int H, float* out, float* tgt);
void launch_fs2_pitch_tail(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                           const float* w, const float* bias, const int* mel2ph, const float* f0_in, const float* uv_in, int norm,
                           float f0_mean, float f0_std, int use_uv, const float* origin, const float* table, int H, float* pitch_pred,
                           float* f0_denorm, int* coarse, float* decoder_inp);

namespace {

constexpr int FS2_REL_MAX_LEN = 5000, FS2_TABLE_INIT = 2000, FS2_MIDI_ROWS = 300, FS2_PITCH_ROWS = 300, FS2_PITCH_TABLE_INIT = 4096;
constexpr int FS2_ENERGY_ROWS = 256, FS2_SPK_VEC = 256;
constexpr float FS2_EPS = 1e-5f;

// RelPositionalEncoding's table (espnet_positional_embedding.py:24-45 with reverse = True) in fp32: row i holds position
// max_len - 1 - i, sin on the even columns and cos on the odd ones
std::vector<float> rel_pos_table(int max_len, int dim) {
    std::vector<float> div(dim / 2), tab((size_t)max_len * dim);
    const float step = (float)-(std::log(10000.0) / (double)dim);
    for (int j = 0; j < dim / 2; ++j) div[j] = std::exp((float)(2 * j) * step);
    for (int i = 0; i < max_len; ++i)
        for (int j = 0; j < dim / 2; ++j) {
            const float a = (float)(max_len - 1 - i) * div[j];
            tab[(size_t)i * dim + 2 * j] = std::sin(a);
            tab[(size_t)i * dim + 2 * j + 1] = std::cos(a);
        }
    return tab;
}

struct FFTLayer {
    float *ln1w, *ln1b, *ln2w, *ln2b;
    PackedW in_proj, out_proj, ffn1, ffn2;
};

// FFTBlocks from the first mask on (tts_modules.py:320-326): EncSALayer x n, the last LayerNorm, each times the mask
struct FFTBlocks {
    std::vector<FFTLayer> layers;
    float *lnw = nullptr, *lnb = nullptr;
    int H = 0, heads = 0, kernel = 0;

    void build(WeightStore& ws, const StateDict& sd, const std::string& name, int n_layers, int hidden, int n_heads, int k) {
        H = hidden;
        heads = n_heads;
        kernel = k;
        const float s = 1.f / std::sqrt((float)k);
        for (int i = 0; i < n_layers; ++i) {
            const std::string p = name + ".layers." + std::to_string(i) + ".op.";
            FFTLayer l;
            MAA_CHECK(get(sd, p + "layer_norm1.weight").numel() == H && get(sd, p + "layer_norm2.weight").numel() == H, "FFTBlocks LayerNorm shape " + p);
            l.ln1w = ws.vec(sd, p + "layer_norm1.weight");
            l.ln1b = ws.vec(sd, p + "layer_norm1.bias");
            l.ln2w = ws.vec(sd, p + "layer_norm2.weight");
            l.ln2b = ws.vec(sd, p + "layer_norm2.bias");
            l.in_proj = ws.pack_conv(sd, p + "self_attn.in_proj_weight", "", 1, 1);
            l.out_proj = ws.pack_conv(sd, p + "self_attn.out_proj.weight", "", 1, 1);
            MAA_CHECK(l.in_proj.N == 3 * H && l.in_proj.K == H && l.out_proj.N == H && l.out_proj.K == H, "FFTBlocks attention shape " + p);
            l.ffn1 = ws.pack_conv(sd, p + "ffn.ffn_1.weight", "", 1, k);
            MAA_CHECK(l.ffn1.N == 4 * H && l.ffn1.K == k * H, "FFTBlocks ffn_1 shape " + p);
            const HostTensor& b1 = get(sd, p + "ffn.ffn_1.bias");
            MAA_CHECK(b1.numel() == 4 * H, "FFTBlocks ffn_1 bias shape " + p);
            std::vector<float> hb(l.ffn1.Npad, 0.f);
            for (int c = 0; c < 4 * H; ++c) hb[c] = b1.data[c] * s;          // gelu((conv + b) * s) = gelu(s * conv + s * b)
            l.ffn1.bias = ws.upload(hb);
            l.ffn2 = ws.pack_conv(sd, p + "ffn.ffn_2.weight", p + "ffn.ffn_2.bias", 1, 1);
            MAA_CHECK(l.ffn2.N == H && l.ffn2.K == 4 * H, "FFTBlocks ffn_2 shape " + p);
            layers.push_back(l);
        }
        MAA_CHECK(get(sd, name + ".layer_norm.weight").numel() == H, "FFTBlocks last LayerNorm shape " + name);
        lnw = ws.vec(sd, name + ".layer_norm.weight");
        lnb = ws.vec(sd, name + ".layer_norm.bias");
    }

    // x [B*T, H], already times nonpad, is overwritten; out [B*T, H].  nonpad / hidden [B*T]: 1 / 0 and 0 / 1 on a live / padding row
    void forward(Ctx& ctx, float* x, int B, int T, const float* nonpad, const float* hidden, float* out) const {
        const long long rows = (long long)B * T;
        const int dh = H / heads;
        float* a = ctx.ws.alloc_f((size_t)rows * H);
        float* y = ctx.ws.alloc_f((size_t)rows * H);
        float* wide = ctx.ws.alloc_f((size_t)rows * 4 * H);          // qkv [rows, 3H], then the FFN's [rows, 4H]
        for (const FFTLayer& l : layers) {
            launch_layernorm(ctx, x, rows, H, l.ln1w, l.ln1b, FS2_EPS, a);
            linear_into(ctx, a, H, rows, H, l.in_proj, nullptr, 0, wide, 3 * H);
            attention_into(ctx, wide, 3 * H, dh, wide + H, 3 * H, dh, wide + 2 * H, 3 * H, dh, B, heads, dh, T, T,
                           1.f / std::sqrt((float)dh), a, H, 0, 0, hidden);
            linear_into(ctx, a, H, rows, H, l.out_proj, x, H, y, H);
            launch_pe_affine_mask(ctx, y, rows, H, nullptr, nullptr, nonpad, x);
            launch_layernorm(ctx, x, rows, H, l.ln2w, l.ln2b, FS2_EPS, a);
            conv1d_act(ctx, a, H, l.ffn1, kernel, B, T, 3, 1.f / std::sqrt((float)kernel), wide);
            linear_into(ctx, wide, 4 * H, rows, 4 * H, l.ffn2, x, H, y, H);
            launch_pe_affine_mask(ctx, y, rows, H, nullptr, nullptr, nonpad, x);
        }
        launch_layernorm(ctx, x, rows, H, lnw, lnb, FS2_EPS, y);
        launch_pe_affine_mask(ctx, y, rows, H, nullptr, nullptr, nonpad, out);
    }
};

}  // namespace

struct FastSpeech2MIDI::Impl {
    maa_fs2_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    int Cp = 0;                          // predictor width
    FFTBlocks enc, dec;
    float *embed = nullptr, *midi = nullptr, *dur_w = nullptr, *dur_b = nullptr, *slur = nullptr, *rel_pe = nullptr;
    ConvPredictor dp;
    PackedW mel_out;
    float alpha = 1.f;
    SinusoidTable table;                 // the decoder's, [max(2000, T_mel + 1), hidden_size]
    // ---- the plain FastSpeech2 only (cfg.plain): no note terms; counted sinusoid positions unless rel_pos; speakers; energy
    SinusoidTable enc_table;             // the encoder's, [max(2000, T + 1), hidden_size] (rel_pos 0)
    float *spk = nullptr, *spk_dur = nullptr, *spk_f0 = nullptr;      // [num_spk + 1, H] each (use_spk_id; the last two with split)
    PackedW spk_proj;                    // Linear(256, H) (use_spk_embed)
    ConvPredictor ep;                    // EnergyPredictor: a PitchPredictor with odim 1 (use_energy_embed)
    float* energy_embed = nullptr;       // [256, H]
    float energy_alpha = 1.f;
    SinusoidTable energy_table;          // the predictor's, [max(4096, T_mel + 1), hidden_size]

    void build(const StateDict& sd) {
        const int H = cfg.hidden_size;
        const HostTensor& e = get(sd, "encoder.embed_tokens.weight");
        MAA_CHECK(e.numel() == (long long)cfg.vocab_size * H, "FastSpeech2MIDI: encoder.embed_tokens.weight must be [vocab_size, hidden_size]");
        embed = ws.vec(sd, "encoder.embed_tokens.weight");
        if (cfg.plain) {
            build_plain(sd);
        } else {
            MAA_CHECK(get(sd, "midi_embed.weight").numel() == (long long)FS2_MIDI_ROWS * H && get(sd, "is_slur_embed.weight").numel() == 2LL * H &&
                          get(sd, "midi_dur_layer.weight").numel() == H && get(sd, "midi_dur_layer.bias").numel() == H,
                      "FastSpeech2MIDI: midi_embed [300, H], midi_dur_layer [H, 1] + [H], is_slur_embed [2, H]");
            midi = ws.vec(sd, "midi_embed.weight");
            dur_w = ws.vec(sd, "midi_dur_layer.weight");
            dur_b = ws.vec(sd, "midi_dur_layer.bias");
            slur = ws.vec(sd, "is_slur_embed.weight");
        }
        if (cfg.rel_pos) rel_pe = ws.upload(rel_pos_table(FS2_REL_MAX_LEN, H));
        enc.build(ws, sd, "encoder", cfg.enc_layers, H, cfg.num_heads, cfg.enc_ffn_kernel_size);
        dec.build(ws, sd, "decoder", cfg.dec_layers, H, cfg.num_heads, cfg.dec_ffn_kernel_size);
        dp.build(ws, sd, "DurationPredictor", "dur_predictor.", cfg.dur_predictor_layers, cfg.dur_predictor_kernel, H, Cp, 1);
        mel_out = ws.pack_conv(sd, "mel_out.weight", "mel_out.bias", 1, 1);
        MAA_CHECK(mel_out.N == cfg.audio_num_mel_bins && mel_out.K == H, "FastSpeech2MIDI: mel_out must be [audio_num_mel_bins, hidden_size]");
        alpha = get(sd, "decoder.pos_embed_alpha").data[0];
        // (encoder_embed_tokens.weight is encoder.embed_tokens.weight again; decoder.embed_positions._float_tensor is bookkeeping)
        table.build(ws, FS2_TABLE_INIT, H);
    }

    // what the plain FastSpeech2 has beside the shared layers (fs2.py:41-47, 65-72)
    void build_plain(const StateDict& sd) {
        const int H = cfg.hidden_size;
        if (!cfg.rel_pos) enc_table.build(ws, FS2_TABLE_INIT, H);
        if (cfg.use_spk_id) {
            const long long n = ((long long)cfg.num_spk + 1) * H;
            MAA_CHECK(get(sd, "spk_embed_proj.weight").numel() == n, "FastSpeech2: spk_embed_proj.weight must be [num_spk + 1, hidden_size]");
            spk = spk_dur = spk_f0 = ws.vec(sd, "spk_embed_proj.weight");
            if (cfg.use_split_spk_id) {
                MAA_CHECK(get(sd, "spk_embed_dur.weight").numel() == n && get(sd, "spk_embed_f0.weight").numel() == n,
                          "FastSpeech2: spk_embed_dur.weight / spk_embed_f0.weight must be [num_spk + 1, hidden_size]");
                spk_dur = ws.vec(sd, "spk_embed_dur.weight");
                spk_f0 = ws.vec(sd, "spk_embed_f0.weight");
            }
        } else if (cfg.use_spk_embed) {
            spk_proj = ws.pack_conv(sd, "spk_embed_proj.weight", "spk_embed_proj.bias", 1, 1);
            MAA_CHECK(spk_proj.N == H && spk_proj.K == FS2_SPK_VEC, "FastSpeech2: spk_embed_proj must be Linear(256, hidden_size)");
        }
        if (cfg.use_energy_embed) {
            MAA_CHECK(get(sd, "energy_embed.weight").numel() == (long long)FS2_ENERGY_ROWS * H, "FastSpeech2: energy_embed.weight must be [256, hidden_size]");
            energy_embed = ws.vec(sd, "energy_embed.weight");
            ep.build(ws, sd, "FastSpeech2 EnergyPredictor", "energy_predictor.", cfg.predictor_layers, cfg.predictor_kernel, H, Cp, 1);
            energy_alpha = get(sd, "energy_predictor.pos_embed_alpha").data[0];
            energy_table.build(ws, FS2_PITCH_TABLE_INIT, H);
        }
    }

    // the duration predictor on dur_inp (its padding rows are 0), then the frame totals      (tts_modules.py:98-118)
    void durations(Ctx& ctx, const float* dur_inp, const float* nonpad, int B, int T, float* xs, int* dur, int* totals) {
        const int H = cfg.hidden_size;
        const long long rows = (long long)B * T;
        const size_t wide = (size_t)rows * (H > Cp ? H : Cp);
        float* a = ctx.ws.alloc_f(wide);
        float* b = ctx.ws.alloc_f(wide);
        const float* y = dp.run(ctx, dur_inp, B, T, nonpad, a, b);
        launch_fs2_dur_head(ctx, y, rows, Cp, dp.gamma(), dp.beta(), dp.EPS, dp.lin_w, dp.lin_b, nonpad, xs, dur);
        launch_fs2_length(ctx, dur, B, T, totals, 0, nullptr);
    }

    // FastSpeech2.forward up to add_dur (fs2.py:84-116): spk_dur [B, H] or null
    void encode_plain(Ctx& ctx, const int* tok, const float* spk_dur_vec, int B, int T, float* encoder_out, float* xs, int* dur,
                      int* totals) {
        const int H = cfg.hidden_size;
        const long long rows = (long long)B * T;
        float* nonpad = ctx.ws.alloc_f((size_t)rows);
        float* hidden = ctx.ws.alloc_f((size_t)rows);
        float* x = ctx.ws.alloc_f((size_t)rows * H);
        launch_fs2_embed_plain(ctx, tok, embed, cfg.vocab_size, cfg.rel_pos ? rel_pe : enc_table.ptr(), std::sqrt((float)H), cfg.rel_pos,
                               B, T, H, x, nonpad, hidden);
        enc.forward(ctx, x, B, T, nonpad, hidden, encoder_out);
        const float* dur_inp = encoder_out;
        if (spk_dur_vec) {
            launch_fs2_add_speaker(ctx, encoder_out, spk_dur_vec, nullptr, nonpad, B, T, H, x);      // (x is free again)
            dur_inp = x;
        }
        durations(ctx, dur_inp, nonpad, B, T, xs, dur, totals);
    }

    // ids int32 [3, B] or vec [B, 256], by the handle's mode -> out [3, B, H] = spk, spk_dur, spk_f0      (fs2.py:96-110)
    void speaker(Ctx& ctx, const int* ids, const float* vec, int B, float* out) {
        const int H = cfg.hidden_size;
        if (cfg.use_spk_id) {
            launch_fs2_speaker_gather(ctx, spk, spk_dur, spk_f0, ids, cfg.use_split_spk_id, cfg.num_spk + 1, B, H, out);
        } else {
            float* p = ctx.ws.alloc_f((size_t)B * H);
            linear_into(ctx, vec, FS2_SPK_VEC, B, FS2_SPK_VEC, spk_proj, nullptr, 0, p, H);
            launch_fs2_speaker_gather(ctx, p, p, p, nullptr, 0, B, B, H, out);
        }
    }

    // add_energy and the last line of the variance stage (fs2.py:128-132, 165-172)
    void finish(Ctx& ctx, const float* pred_inp, const float* acc, const int* mel2ph, const float* energy, const float* spk_vec, int B,
                int T_mel, float* decoder_inp, float* energy_pred, int* energy_bin) {
        const int H = cfg.hidden_size;
        const long long rows = (long long)B * T_mel;
        const float* y = nullptr;
        if (cfg.use_energy_embed) {
            const size_t wide = (size_t)rows * (H > Cp ? H : Cp);
            float* a = ctx.ws.alloc_f(wide);
            float* b = ctx.ws.alloc_f(wide);
            launch_pe_pos_add(ctx, pred_inp, B, T_mel, H, energy_table.ptr(), energy_alpha, b);
            y = ep.run(ctx, b, B, T_mel, nullptr, a, b);
        }
        launch_fs2_energy_tail(ctx, y, rows, Cp, y ? ep.gamma() : nullptr, y ? ep.beta() : nullptr, ep.EPS, ep.lin_w, ep.lin_b, mel2ph,
                               energy, acc, energy_embed, spk_vec, T_mel, H, energy_pred, energy_bin, decoder_inp);
    }

    void encode(Ctx& ctx, const int* tok, const int* pitch_midi, const float* midi_dur, const int* is_slur, int B, int T,
                float* encoder_out, float* xs, int* dur, int* totals) {
        const int H = cfg.hidden_size;
        const long long rows = (long long)B * T;
        float* nonpad = ctx.ws.alloc_f((size_t)rows);
        float* hidden = ctx.ws.alloc_f((size_t)rows);
        float* x = ctx.ws.alloc_f((size_t)rows * H);
        launch_fs2_embed(ctx, tok, pitch_midi, midi_dur, is_slur, embed, cfg.vocab_size, midi, dur_w, dur_b, slur, rel_pe,
                         std::sqrt((float)H), B, T, H, x, nonpad, hidden);
        enc.forward(ctx, x, B, T, nonpad, hidden, encoder_out);
        durations(ctx, encoder_out, nonpad, B, T, xs, dur, totals);      // on encoder_out * src_nonpadding: its padding rows are 0 already
    }

    void decode(Ctx& ctx, const float* encoder_out, const int* mel2ph, int B, int T, int T_mel, float* decoder_inp, float* mel) {
        const int H = cfg.hidden_size;
        const long long rows = (long long)B * T_mel;
        float* tgt = ctx.ws.alloc_f((size_t)rows);
        launch_fs2_expand(ctx, encoder_out, mel2ph, B, T, T_mel, H, decoder_inp, tgt);
        if (mel) decoder(ctx, decoder_inp, tgt, B, T_mel, mel);
    }

    // FastSpeech2.run_decoder (fs2.py:222-226) on a decoder_inp some other stage finished (the pitch branch): tgt from mel2ph
    void run_decoder(Ctx& ctx, const float* decoder_inp, const int* mel2ph, int B, int T_mel, float* mel) {
        const long long rows = (long long)B * T_mel;
        float* tgt = ctx.ws.alloc_f((size_t)rows);
        launch_fs2_tgt_mask(ctx, mel2ph, rows, tgt);
        decoder(ctx, decoder_inp, tgt, B, T_mel, mel);
    }

    // decoder_inp [B*T_mel, H], tgt [B*T_mel] = (mel2ph > 0) -> mel [B*T_mel, M]
    void decoder(Ctx& ctx, const float* decoder_inp, const float* tgt, int B, int T_mel, float* mel) {
        const int H = cfg.hidden_size, M = cfg.audio_num_mel_bins;
        const long long rows = (long long)B * T_mel;
        // ---- FastspeechDecoder: mask from the data, positions counted on it      (tts_modules.py:313-320)
        float* nonpad = ctx.ws.alloc_f((size_t)rows);
        float* hidden = ctx.ws.alloc_f((size_t)rows);
        float* x = ctx.ws.alloc_f((size_t)rows * H);
        float* y = ctx.ws.alloc_f((size_t)rows * H);
        launch_pe_frame_mask(ctx, decoder_inp, rows, H, nonpad, hidden);
        launch_pe_pos_add(ctx, decoder_inp, B, T_mel, H, table.ptr(), alpha, x);
        launch_pe_affine_mask(ctx, x, rows, H, nullptr, nullptr, nonpad, x);
        dec.forward(ctx, x, B, T_mel, nonpad, hidden, y);
        linear_into(ctx, y, H, rows, H, mel_out, nullptr, 0, mel, M);
        launch_pe_affine_mask(ctx, mel, rows, M, nullptr, nullptr, tgt, mel);
    }
};

FastSpeech2MIDI::FastSpeech2MIDI(const maa_fs2_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    impl_->cfg = cfg;
    impl_->Cp = cfg.predictor_hidden > 0 ? cfg.predictor_hidden : cfg.hidden_size;
    impl_->build(sd);
}
FastSpeech2MIDI::~FastSpeech2MIDI() = default;
const maa_fs2_config& FastSpeech2MIDI::config() const { return impl_->cfg; }

void FastSpeech2MIDI::encode(Ctx& ctx, const int* tokens, const int* pitch_midi, const float* midi_dur, const int* is_slur, int B, int T,
                             float* encoder_out, float* xs, int* dur, int* totals) {
    Impl& m = *impl_;
    MAA_CHECK(!m.cfg.plain, "maa_fs2_encode: this handle is the plain FastSpeech2 (plain = 1), which has no note features -- call maa_fs2_encode_plain");
    MAA_CHECK(T <= FS2_REL_MAX_LEN, "FastSpeech2MIDI: more tokens than RelPositionalEncoding's max_len (5000)");
    PrecisionGuard pg(ctx, m.precision);
    run_sized(ctx, [&] { m.encode(ctx, tokens, pitch_midi, midi_dur, is_slur, B, T, encoder_out, xs, dur, totals); });
}

void FastSpeech2MIDI::encode_plain(Ctx& ctx, const int* tokens, const float* spk_dur, int B, int T, float* encoder_out, float* xs,
                                   int* dur, int* totals) {
    Impl& m = *impl_;
    MAA_CHECK(m.cfg.plain, "maa_fs2_encode_plain: this handle is FastSpeech2MIDI (plain = 0), whose encoder adds the note features -- call maa_fs2_encode");
    MAA_CHECK(!m.cfg.rel_pos || T <= FS2_REL_MAX_LEN, "FastSpeech2: more tokens than RelPositionalEncoding's max_len (5000)");
    PrecisionGuard pg(ctx, m.precision);
    if (!m.cfg.rel_pos) m.enc_table.grow(ctx, T);
    run_sized(ctx, [&] { m.encode_plain(ctx, tokens, spk_dur, B, T, encoder_out, xs, dur, totals); });
}

void FastSpeech2MIDI::speaker(Ctx& ctx, const int* ids, const float* vec, int B, float* out) {
    Impl& m = *impl_;
    MAA_CHECK(m.cfg.plain && (m.cfg.use_spk_id || m.cfg.use_spk_embed),
              "maa_fs2_speaker: this handle has no speaker embedding (neither use_spk_id nor use_spk_embed)");
    MAA_CHECK(m.cfg.use_spk_id ? ids != nullptr : vec != nullptr,
              m.cfg.use_spk_id ? "maa_fs2_speaker: a use_spk_id handle needs d_ids" : "maa_fs2_speaker: a use_spk_embed handle needs d_vec");
    PrecisionGuard pg(ctx, m.precision);
    run_sized(ctx, [&] { m.speaker(ctx, ids, vec, B, out); });
}

void FastSpeech2MIDI::add_speaker(Ctx& ctx, const float* x, const float* spk, const int* mel2ph, int B, int T_mel, float* out) {
    Impl& m = *impl_;
    run_sized(ctx, [&] { launch_fs2_add_speaker(ctx, x, spk, mel2ph, nullptr, B, T_mel, m.cfg.hidden_size, out); });
}

void FastSpeech2MIDI::finish(Ctx& ctx, const float* pred_inp, const float* acc, const int* mel2ph, const float* energy, const float* spk,
                             int B, int T_mel, float* decoder_inp, float* energy_pred, int* energy_bin) {
    Impl& m = *impl_;
    MAA_CHECK(!m.cfg.use_energy_embed || pred_inp, "maa_fs2_finish: a use_energy_embed handle needs d_pred_inp, the energy predictor's input");
    PrecisionGuard pg(ctx, m.precision);
    if (m.cfg.use_energy_embed) m.energy_table.grow(ctx, T_mel);
    run_sized(ctx, [&] { m.finish(ctx, pred_inp, acc, mel2ph, energy, spk, B, T_mel, decoder_inp, energy_pred, energy_bin); });
}

void FastSpeech2MIDI::length_regulate(Ctx& ctx, const int* dur, int B, int T, int T_mel, int* mel2ph) {
    run_sized(ctx, [&] { launch_fs2_length(ctx, dur, B, T, nullptr, T_mel, mel2ph); });
}

void FastSpeech2MIDI::decode(Ctx& ctx, const float* encoder_out, const int* mel2ph, int B, int T, int T_mel, float* decoder_inp,
                             float* mel_out) {
    Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    if (mel_out) m.table.grow(ctx, T_mel);
    run_sized(ctx, [&] { m.decode(ctx, encoder_out, mel2ph, B, T, T_mel, decoder_inp, mel_out); });
}

void FastSpeech2MIDI::run_decoder(Ctx& ctx, const float* decoder_inp, const int* mel2ph, int B, int T_mel, float* mel_out) {
    Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    m.table.grow(ctx, T_mel);
    run_sized(ctx, [&] { m.run_decoder(ctx, decoder_inp, mel2ph, B, T_mel, mel_out); });
}

// ---- the pitch branch of the cascade configurations (use_pitch_embed, pitch_type 'frame'): fs2.py:56-64,125-128,174-220
struct FS2Pitch::Impl {
    maa_fs2_pitch_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    int Cp = 0;                          // predictor width
    float* embed = nullptr;              // pitch_embed.weight [300, H]
    ConvPredictor pp;
    float alpha = 1.f;
    SinusoidTable table;                 // the predictor's, [max(4096, T_mel + 1), hidden_size]

    void build(const StateDict& sd) {
        const int H = cfg.hidden_size;
        MAA_CHECK(get(sd, "pitch_embed.weight").numel() == (long long)FS2_PITCH_ROWS * H, "FastSpeech2MIDI pitch: pitch_embed.weight must be [300, hidden_size]");
        embed = ws.vec(sd, "pitch_embed.weight");
        pp.build(ws, sd, "FastSpeech2MIDI PitchPredictor", "pitch_predictor.", cfg.predictor_layers, cfg.predictor_kernel, H, Cp, 2);
        alpha = get(sd, "pitch_predictor.pos_embed_alpha").data[0];
        // (pitch_predictor.embed_positions._float_tensor is bookkeeping: not read)
        table.build(ws, FS2_PITCH_TABLE_INIT, H);
    }

    void forward(Ctx& ctx, const float* pred_inp, const float* origin, const int* mel2ph, const float* f0, const float* uv, int B, int T_mel,
                 float* decoder_inp, float* pitch_pred, float* f0_denorm, int* coarse) {
        const int H = cfg.hidden_size;
        const long long rows = (long long)B * T_mel;
        const size_t wide = (size_t)rows * (H > Cp ? H : Cp);
        float* a = ctx.ws.alloc_f(wide);
        float* b = ctx.ws.alloc_f(wide);
        // ---- PitchPredictor (tts_modules.py:247-260) on pitch_inp (0 where mel2ph is 0 already): origin itself without speakers,
        // (origin + spk_f0) * tgt with them; no mask between its layers
        launch_pe_pos_add(ctx, pred_inp, B, T_mel, H, table.ptr(), alpha, b);
        const float* y = pp.run(ctx, b, B, T_mel, nullptr, a, b);          // (a LayerNorm writes over b, which its convolution has read)
        launch_fs2_pitch_tail(ctx, y, rows, Cp, pp.gamma(), pp.beta(), pp.EPS, pp.lin_w, pp.lin_b, mel2ph, f0, uv, cfg.pitch_norm,
                              cfg.f0_mean, cfg.f0_std, cfg.use_uv, origin, embed, H, pitch_pred, f0_denorm, coarse, decoder_inp);
    }
};

FS2Pitch::FS2Pitch(const maa_fs2_pitch_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    impl_->cfg = cfg;
    impl_->Cp = cfg.predictor_hidden > 0 ? cfg.predictor_hidden : cfg.hidden_size;
    impl_->build(sd);
}
FS2Pitch::~FS2Pitch() = default;
const maa_fs2_pitch_config& FS2Pitch::config() const { return impl_->cfg; }

void FS2Pitch::forward(Ctx& ctx, const float* pred_inp, const float* origin, const int* mel2ph, const float* f0, const float* uv, int B,
                       int T_mel, float* decoder_inp, float* pitch_pred, float* f0_denorm, int* coarse) {
    Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    m.table.grow(ctx, T_mel);
    run_sized(ctx, [&] { m.forward(ctx, pred_inp, origin, mel2ph, f0, uv, B, T_mel, decoder_inp, pitch_pred, f0_denorm, coarse); });
}

}  // namespace maa
