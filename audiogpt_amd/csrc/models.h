// Model executors behind the C ABI handles.  Each owns its Impl through a unique_ptr: a constructor that throws (a state dict
// without a key) frees what it had built, and the destructors, declared here, are defined where Impl is complete.
#pragma once
#include "../../include/maa.h"
#include "blocks.h"

#include <memory>

namespace maa {

// A guided DDIM step evaluates the model on cat([x] * 2) with cat([uncond, cond]) (ddim.py:177-199): the halves are the same tensor
// before the first cross-attention, so those layers need computing once.  How one forward takes part in that:
//   None    the whole network
//   Dup     the batch is cat([x] * 2) on one stream -- samples [B/2, B) repeat [0, B/2): those layers run on one half, and their
//           outputs are duplicated where the halves part
//   Export  the unconditional lane (batch_off 0): the whole network, and it leaves those layers' outputs in its workspace
//   Import  the conditional lane (batch_off B), called after Export with the same CfgPrefix: starts from them
enum class CfgShare { None, Dup, Export, Import };
// What the Export forward hands to the Import forward of the same step.  The step owns it (ddim.cpp Loop::forward, one per
// call) and supplies `ready`, which orders the importing stream behind the exporting one; the step's join orders the next step's
// writes behind the reads.  hs0: conv_in's output (the first skip tensor); xres, y1, q: the first transformer's input, its
// residual stream after attn1 and attn2's queries -- all in the exporting context's workspace.
struct CfgPrefix {
    const float *hs0 = nullptr, *xres = nullptr, *y1 = nullptr, *q = nullptr;
    int B = 0, H = 0, W = 0;
    bool filled = false;
    hipEvent_t ready = nullptr;
};

// What holds for one UNet forward only.
// emb_row: the ResBlocks' time-embedding row of this step from emb_table() (one row for all samples: every sample of a DDIM
//   step shares t); null: computed from t (and, I2A, the context) as the reference does per forward
// batch_off >= 0: this call covers samples [batch_off, batch_off + B) of the batch set_context saw (one lane of a CFG step);
//   x / t / out already point at that sample, the context rows and the cross-attention K/V caches are offset inside
// mode (with emb_row only), prefix (Export / Import only): see CfgShare.  A UNet the hand-over is not written for (unet.cpp
//   prefix_ok) runs the whole network in both lanes.
struct UNetForwardOpt {
    const float* emb_row = nullptr;
    int batch_off = -1;
    CfgShare mode = CfgShare::None;
    CfgPrefix* prefix = nullptr;
};

class UNet {
public:
    // precision: 0 exact fp32 MFMA, 1 bf16x3 split, 2 plain bf16 operands (fixed at creation: it decides the
    // packed weight layout)
    UNet(const maa_unet_config& cfg, const StateDict& sd, int precision);
    ~UNet();
    // rep > 1: the B samples are evaluated as B * rep rows, sample b's conditioning serving rows b * rep .. b * rep + rep - 1 (the
    // crops of split_input_params); the K/V projections are still computed once per sample and copied on the device
    void set_context(Ctx& ctx, const float* d_context, int B, int L, int rep = 1);
    int context_len() const;      // tokens per sample of the last set_context (0: none yet)
    // classifier-free guidance: context rows [uncond (B) ; cond (B)] assembled in a buffer the UNet owns (it stays
    // valid for later forwards, e.g. the I2A time-embedding add), then set_context over 2B rows
    void set_context_cfg(Ctx& ctx, const float* d_uncond, const float* d_cond, int B, int L, int rep = 1);
    void forward(Ctx& ctx, const float* x_nchw, const float* t, const float* context, int B, int H, int W, float* out_nchw,
                 const UNetForwardOpt& opt = UNetForwardOpt());
    // Linear(SiLU(time_embed(timestep_embedding(t)))) of every ResBlock for `rows` timesteps at once -> [rows, emb_width()]
    // (openaimodel.py:725-726, 218-224): the sampling loop computes its S rows once instead of per step.  Not for the
    // I2A variant, whose embedding also takes the sample's context (custom_openaimodel.py:352-354).
    void emb_table(Ctx& ctx, const float* d_t, int rows, float* d_out);
    int emb_width() const;
    const maa_unet_config& config() const;
    size_t weight_bytes() const;
    // context pointer remembered by set_context (needed by the I2A time-embedding add)
    const float* context_ptr = nullptr;
    // addresses / sizes of the UNet-owned buffers a captured forward reads (cross-attention K/V caches, CFG context):
    // appended to a graph cache key
    void graph_key(std::vector<unsigned long long>& key) const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

class VAE {
public:
    VAE(const maa_vae_config& cfg, const StateDict& sd, int precision);
    ~VAE();
    void decode(Ctx& ctx, const float* z_nchw, int B, int h, int w, float inv_scale, float* mel_nchw);
    // decode + the tools' clamp((mel + 1) / 2, 0, 1) (audio-chatgpt.py:175-176) in the last pass: spec [B, 8h, 8w]
    void decode_spec(Ctx& ctx, const float* z_nchw, int B, int h, int w, float inv_scale, float* spec);
    void encode_moments(Ctx& ctx, const float* mel_nchw, int B, int H, int W, float* moments_nchw);
    const maa_vae_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

class Vocoder {
public:
    Vocoder(const maa_vocoder_config& cfg, const StateDict& sd, int precision);
    ~Vocoder();
    void forward(Ctx& ctx, const float* mel, int B, int T, float* wav);
    // NSF branch: f0 [B, T], rand_ini [B, harmonics+1], noise [B, T*hop, harmonics+1] (see maa.h)
    void forward_f0(Ctx& ctx, const float* mel, const float* f0, const float* rand_ini, const float* noise, int B, int T,
                    float* wav);
    int hop() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

class DiffNet {
public:
    DiffNet(const maa_diffnet_config& cfg, const StateDict& sd, int precision);
    ~DiffNet();
    void forward(Ctx& ctx, const float* spec, const float* t, const float* cond, int B, int T, float* out);
    void plms_sample(Ctx& ctx, const maa_plms_args& a, float* d_x);
    // the ancestral chain (shallow_diffusion_tts.py:159-166, 269-271): steps a.start .. a.start - a.n + 1 on the device
    void ddpm_sample(Ctx& ctx, const maa_ds_ddpm_args& a, float* d_x);
    const maa_diffnet_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// The Glow post-net of GenerSpeech / PortaSpeech in reverse (glow.cpp, glow.hip): latent + conditioning -> mel
class Glow {
public:
    Glow(const maa_glow_config& cfg, const StateDict& sd, int precision);
    ~Glow();
    // z [B, T, C], g [B, T, gin] (null exactly when gin_channels == 0), mask [B, T] of 0 / 1 (null: all ones) -> x [B, 2 (T / 2), C];
    // logdet [B] and hiddens [3 n_blocks, B, T / 2, 2C] (every flow's output in execution order, squeezed rows) optional
    void reverse(Ctx& ctx, const float* z, const float* g, const float* mask, int B, int T, float* x, float* logdet, float* hiddens);
    const maa_glow_config& config() const;      // zero fields resolved

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};
// the checks of maa_glow_create / maa_glow_reverse that touch no device (api.cpp calls them before it binds the context)
maa_glow_config glow_resolved(const maa_glow_config& cfg);      // a zero size field -> GenerSpeech's shipped value (maa.h)
void check_glow_config(const maa_glow_config& cfg);
void check_glow_reverse_args(const void* glow, const float* d_z, int B, int T, const float* d_x);
// Row launches of glow.hip (the kernels carry the formulas): C, H and gin multiples of 4, every pointer 16-byte aligned
void launch_glow_squeeze(const Ctx& ctx, const float* in, const float* mask, int B, int T, int C, float* out, float* mask_out);
void launch_glow_gate(const Ctx& ctx, const float* y, long long rows, int H, float* z);
void launch_glow_wn_residual(const Ctx& ctx, const float* rs, long long rows, int H, const float* mask, bool first, bool last, float* x,
                             float* skip);
void launch_glow_block_tail(const Ctx& ctx, const float* x, const float* eo, const float* mask, long long rows, int C, int sigmoid_scale,
                            const float* winv, const float* an_bias, const float* an_einv, bool first, float* out, float* rowld,
                            float* h_cpl, float* h_inv, float* h_act);
void launch_glow_logdet(const Ctx& ctx, const float* rowld, const float* mask, int B, int Ts, float per_len, float* logdet);

// DiffSinger's PitchExtractor (pitch_extractor.cpp, pitch.hip): the generated mel -> f0 for the NSF vocoder
class PitchExtractor {
public:
    PitchExtractor(const maa_pitch_extractor_config& cfg, const StateDict& sd, int precision);
    ~PitchExtractor();
    // mel [B, T, n_mel_bins] -> pitch_pred [B, T, 2], f0 [B, T]; hidden_out (optional) [B, T, hidden_size]: pitch_predictor's input
    void forward(Ctx& ctx, const float* mel, int B, int T, float* pitch_pred, float* f0, float* hidden_out);
    const maa_pitch_extractor_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// Row launches of pitch.hip that the extractor and the FastSpeech2 front end share.  Their shared host layers -- the "same"
// Conv1d with an epilogue activation, the sinusoid table, the convolutional predictor stack -- are seq_layers.h's; the device
// code under their LayerNorms and heads is row_device.h's.
// mask[row] = 0 where every channel of the row is +-0, else 1; hidden (optional) [row] = 1 - mask[row], an attention key mask
void launch_pe_frame_mask(const Ctx& ctx, const float* mel, long long rows, int M, float* mask, float* hidden = nullptr);
// out = (x * scale + shift) * mask[row]; scale == nullptr: out = x * mask[row] (out may be x)
void launch_pe_affine_mask(const Ctx& ctx, const float* x, long long rows, int C, const float* scale, const float* shift,
                           const float* mask, float* out);
// out = x + alpha * table[make_positions(x[..., 0])], the positions counted on the device; pos_out (optional) int [B, T] receives
// them in place of the workspace buffer
void launch_pe_pos_add(Ctx& ctx, const float* x, int B, int T, int C, const float* table, float alpha, float* out,
                       int* pos_out = nullptr);
// out = res + relu(GroupNorm(y)), the statistics over all T frames of a sample (out may be y)
void launch_pe_gn_relu_res(Ctx& ctx, const float* y, const float* res, int B, int T, int C, int groups, const float* gamma,
                           const float* beta, float eps, float* out);
// The predictors' last LayerNorm + narrow Linear: Linear(C, 2) and denorm_f0 (pitch.hip), Linear(C, 1), mask and out2dur (fs2.hip)
void launch_pe_head(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                    const float* w, const float* bias, const float* mask, int norm, float f0_mean, float f0_std, int use_uv,
                    float* pitch_pred, float* f0);
void launch_fs2_dur_head(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                         const float* w, const float* bias, const float* nonpad, float* xs, int* dur);
// The plain FastSpeech2's rows and run_decoder's mask (fs2.hip), declared here for fs2.cpp and for maa_op_tts_rows
void launch_fs2_tgt_mask(const Ctx& ctx, const int* mel2ph, long long rows, float* tgt);
void launch_fs2_embed_plain(Ctx& ctx, const int* tok, const float* E, int vocab, const float* pe, float scale, int rel, int B, int T,
                            int H, float* x, float* nonpad, float* hidden);
void launch_fs2_add_speaker(const Ctx& ctx, const float* x, const float* spk, const int* mel2ph, const float* mask, int B, int T, int H,
                            float* out);
void launch_fs2_speaker_gather(const Ctx& ctx, const float* t0, const float* t1, const float* t2, const int* ids, int split, int n_rows,
                               int B, int H, float* out);
void launch_fs2_energy_tail(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                            const float* w, const float* bias, const int* mel2ph, const float* energy_in, const float* acc,
                            const float* table, const float* spk, int T_mel, int H, float* energy_pred, int* energy_bin,
                            float* decoder_inp);

// DiffSinger's FastSpeech2MIDI front end (fs2.cpp, fs2.hip): score -> encoder_out / durations, then mel2ph -> decoder_inp / mel_out
class FastSpeech2MIDI {
public:
    FastSpeech2MIDI(const maa_fs2_config& cfg, const StateDict& sd, int precision);
    ~FastSpeech2MIDI();
    // tokens / pitch_midi / is_slur (optional) int32 [B, T], midi_dur (optional) [B, T] -> encoder_out [B, T, H], xs [B, T],
    // dur int32 [B, T], totals int32 [B]
    void encode(Ctx& ctx, const int* tokens, const int* pitch_midi, const float* midi_dur, const int* is_slur, int B, int T,
                float* encoder_out, float* xs, int* dur, int* totals);
    // The plain FastSpeech2 (cfg.plain; modules/fastspeech/fs2.py): tokens int32 [B, T], spk_dur (optional) [B, H] -> as encode
    void encode_plain(Ctx& ctx, const int* tokens, const float* spk_dur, int B, int T, float* encoder_out, float* xs, int* dur,
                      int* totals);
    // ids int32 [3, B] (use_spk_id) or vec [B, 256] (use_spk_embed), by the handle's mode -> out [3, B, H]: spk, spk_dur, spk_f0
    void speaker(Ctx& ctx, const int* ids, const float* vec, int B, float* out);
    // out [B, T_mel, H] = (x + spk[b]) * (mel2ph > 0): the pitch and energy predictors' input
    void add_speaker(Ctx& ctx, const float* x, const float* spk, const int* mel2ph, int B, int T_mel, float* out);
    // the energy predictor on pred_inp (when the handle has one), then decoder_inp = (acc + energy_embed[bin] + spk[b]) * (mel2ph > 0);
    // energy / spk / energy_pred [B, T_mel] / energy_bin int32 [B, T_mel] optional
    void finish(Ctx& ctx, const float* pred_inp, const float* acc, const int* mel2ph, const float* energy, const float* spk, int B,
                int T_mel, float* decoder_inp, float* energy_pred, int* energy_bin);
    void length_regulate(Ctx& ctx, const int* dur, int B, int T, int T_mel, int* mel2ph);
    // encoder_out [B, T, H], mel2ph int32 [B, T_mel] -> decoder_inp [B, T_mel, H], mel_out (optional) [B, T_mel, mel bins]
    void decode(Ctx& ctx, const float* encoder_out, const int* mel2ph, int B, int T, int T_mel, float* decoder_inp, float* mel_out);
    // decode's second half on a decoder_inp [B, T_mel, H] the caller supplies (run_decoder, fs2.py:222-226) -> mel_out
    void run_decoder(Ctx& ctx, const float* decoder_inp, const int* mel2ph, int B, int T_mel, float* mel_out);
    const maa_fs2_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// The pitch branch the cascade singing configurations add to that front end (fs2.cpp, fs2.hip: use_pitch_embed, pitch_type frame)
class FS2Pitch {
public:
    FS2Pitch(const maa_fs2_pitch_config& cfg, const StateDict& sd, int precision);
    ~FS2Pitch();
    // pred_inp [B, T_mel, H] (the predictor's input: origin itself, or (origin + spk_f0) * tgt), origin [B, T_mel, H] (decode's
    // decoder_inp, which the table row is added to), mel2ph int32 [B, T_mel], f0 / uv (each optional) [B, T_mel] -> decoder_inp
    // [B, T_mel, H], pitch_pred [B, T_mel, 2], f0_denorm [B, T_mel], coarse (optional) int32 [B, T_mel]
    void forward(Ctx& ctx, const float* pred_inp, const float* origin, const int* mel2ph, const float* f0, const float* uv, int B,
                 int T_mel, float* decoder_inp, float* pitch_pred, float* f0_denorm, int* coarse);
    const maa_fs2_pitch_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

class Encoder {
public:
    Encoder(const maa_encoder_config& cfg, const StateDict& sd, int precision);
    ~Encoder();
    void text(Ctx& ctx, const int* d_ids, int B, int L, float* d_out);
    void text_cls(Ctx& ctx, const int* d_ids, int B, int L, float* d_out);
    void image(Ctx& ctx, const float* d_img, int B, float* d_out);
    const maa_encoder_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// CLAP audio branch of the best-of-n scorer: Cnn14 from the log-mel on + Projection, unit-length rows (clap_audio.cpp)
class ClapAudio {
public:
    ClapAudio(const maa_clap_audio_config& cfg, const StateDict& sd, int precision);
    ~ClapAudio();
    void embed(Ctx& ctx, const float* d_logmel, int B, int T, float* d_embedding, float* d_z);
    const maa_clap_audio_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// framed DFT -> |.|^p -> mel filter bank -> log: the 16 kHz front end of the inpainting tool and the 44.1 kHz one of the
// CLAP scorer (clap_audio.cpp); always exact fp32
class Spectral {
public:
    Spectral(const maa_spectral_config& cfg, const float* h_basis, const float* h_melw);
    ~Spectral();
    void forward(Ctx& ctx, const float* d_wav, int B, int n, float* d_out);
    const maa_spectral_config& config() const;

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// torchaudio-style polyphase sinc resampler as one strided FIR-bank contraction (clap_audio.cpp); always exact fp32
class Resampler {
public:
    Resampler(int orig, int neu, int width, int klen, const float* h_kernels);
    ~Resampler();
    long long out_length(long long n) const;
    void forward(Ctx& ctx, const float* d_wav, int B, int n, float* d_out);

private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// ---- shared by the samplers' host code (ddim.cpp, diffnet.cpp)
// n rows of `width` >= 5 floats, the rest zero: {sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, fifth(t)} of the posterior at
// timestep t, the fifth column -- the noise's scale, exp(0.5 logvar[t]) or sigma[t] -- 0 in row 0 (the reference's nonzero_mask)
template <class F>
std::vector<float> posterior_rows(const float* sqrt_recip_ac, const float* sqrt_recipm1_ac, const float* coef1, const float* coef2, int n,
                                  F&& fifth, int width = 5) {
    std::vector<float> tab((size_t)n * width, 0.f);
    for (int t = 0; t < n; ++t) {
        float* r = &tab[(size_t)t * width];
        r[0] = sqrt_recip_ac[t], r[1] = sqrt_recipm1_ac[t], r[2] = coef1[t], r[3] = coef2[t];
        r[4] = t == 0 ? 0.f : fifth(t);
    }
    return tab;
}
void ddim_sample(Ctx& ctx, UNet& unet, const maa_ddim_args& a, float* d_x);
// check_*_args, each declared above the entry it guards: every argument check of that entry that touches no device (api.cpp
// calls it before it binds the context; a malformed call fails the same way with or without a device).  The entries themselves
// do not repeat them.  `unet` is the caller's handle, tested against null only.
// DDIMSampler.decode (ddim.py:243-261): DDIM indices t_start - 1 .. 0 of the S-step schedule `a` describes; d_noise_p holds t_start
// draws in loop order
void check_ddim_decode_args(const void* unet, const maa_ddim_args* a, int t_start, const float* d_x);
void ddim_decode(Ctx& ctx, UNet& unet, const maa_ddim_args& a, int t_start, float* d_x);
// PLMSSampler.plms_sampling (plms.py:115-236) over the S-step schedule `a` describes (eta 0: no sigmas, no step noise)
void check_ldm_plms_args(const void* unet, const maa_ddim_args* a, const float* d_x);
void ldm_plms_sample(Ctx& ctx, UNet& unet, const maa_ddim_args& a, float* d_x);
// LatentDiffusion_audio's ancestral chain (ddpm_audio.py:717-884): DDPM steps a.start .. a.start - a.n + 1 on the device
void check_ddpm_sample_args(const void* unet, const maa_ddpm_args* a, const float* d_x);
void ddpm_sample(Ctx& ctx, UNet& unet, const maa_ddpm_args& a, float* d_x);
// one such step with a timestep per sample and host tables of n_tab rows (p_sample); checks every t[b] against n_tab
void check_ddpm_update_args(const float* d_x, const float* d_eps, const int32_t* d_t, const float* h_sqrt_recip_ac,
                            const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_logvar, int n_tab,
                            const float* d_noise, int B, int C, int H, int W, const float* d_x_prev, const float* d_x_recon);
void ddpm_update(Ctx& ctx, const float* d_x, const float* d_eps, const int32_t* d_t, const float* h_sqrt_recip_ac,
                 const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_logvar, int n_tab,
                 const float* d_noise, float temperature, bool clip, int B, int C, int H, int W, float* d_x_prev, float* d_x_recon);
// DiffSinger's p_sample arithmetic for one step with a timestep per sample (shallow_diffusion_tts.py:134-166), d_x in place;
// host tables of `timesteps` rows; checks every t[b] against them (csrc/diffnet.cpp)
void ds_ddpm_update(Ctx& ctx, const float* d_eps, const float* d_t, const float* d_noise, const float* h_sqrt_recip_ac,
                    const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_sigma, int timesteps,
                    int B, int M, int T, bool clip, float* d_x);
// One model evaluation with split_input_params outside a loop (ddpm_audio.py:572-654): unfold, the UNet over B * L crop rows,
// fold.  h_weight [kh * kw][L] on the host (get_weighting's table); d_context [B, context_len(), context_dim] or null
void unet_forward_split(Ctx& ctx, UNet& unet, const float* d_x, const float* d_t, const float* d_context, int B, int H, int W, int kh,
                        int kw, int sh, int sw, const float* h_weight, float* d_out);
// DDIMSampler.stochastic_encode (ddim.py:227-241) with host tables of n_tab rows; checks every t[b] against n_tab
void check_stochastic_encode_args(const float* d_x0_or_moments, bool from_moments, const float* d_noise_post, const int32_t* d_t,
                                  const float* h_sqrt_a, const float* h_sqrt_1ma, int n_tab, const float* d_noise, int B, int C, int H,
                                  int W, const float* d_out);
void ddim_stochastic_encode(Ctx& ctx, const float* d_x0_or_moments, bool from_moments, float scale_factor, const float* d_noise_post,
                            const int32_t* d_t, const float* h_sqrt_a, const float* h_sqrt_1ma, int n_tab, const float* d_noise, int B,
                            int C, int H, int W, float* d_out);

}  // namespace maa
