/* libaudiogpt_mi355x -- C ABI of the MI355X-native Make-An-Audio generation backend.
 *
 * The reference (AIGC-Audio/AudioGPT) is pure Python/PyTorch and has NO FFI / plugin layer for this path
 * (SURVEY.md 8b): what this header replaces are the Python methods the tool classes call.  Each entry
 * point names the reference interface it stands in for; `INTEGRATION.md` shows the ctypes binding a
 * maintainer adds on the reference side (audiogpt_amd/_lib.py is that binding, shipped).
 *
 * Conventions
 *   - every function returns 0 on success, a negative maa_status otherwise; maa_last_error() returns a
 *     thread-local message.  No C++ exception crosses the boundary.
 *   - tensors are plain pointers + sizes.  Device pointers are fp32 and live on the context's device;
 *     the caller owns every buffer, the library owns only the opaque handles.
 *   - tensor layouts at the boundary are the reference's: images NCHW, mels [B, n_mels, T], waves [B, T*hop],
 *     cross-attention context [B, L, context_dim].  (Inside, activations are channels-last.)
 *   - all launches are asynchronous on the context's HIP stream; only maa_ctx_synchronize blocks.
 *   - one context per (device, stream); calls on one context must be serialised by the caller
 *     (the reference's DDIMSampler is not re-entrant either: ddim.py:27-56 re-registers buffers per call).
 *   - weights are passed as HOST pointers in the reference's state_dict layout (names + shapes + fp32 data);
 *     the library repacks them for its kernels and uploads them.
 */
#ifndef MAA_H_
#define MAA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum maa_status {
    MAA_OK = 0,
    MAA_ERR_INVALID = -1,   /* bad argument / shape / missing weight */
    MAA_ERR_HIP = -2,       /* HIP runtime failure */
    MAA_ERR_INTERNAL = -3
} maa_status;

typedef struct maa_ctx maa_ctx;         /* device + stream + workspace */
typedef struct maa_unet maa_unet;       /* UNetModel weights + plan */
typedef struct maa_vae maa_vae;         /* AutoencoderKL decoder (+ encoder) */
typedef struct maa_vocoder maa_vocoder; /* HiFi-GAN / BigVGAN generator */

/* thread-local message of the last failing call on this thread */
const char* maa_last_error(void);
/* "libaudiogpt_mi355x <version> gfx950" */
const char* maa_version(void);

/* ---- context ------------------------------------------------------------------------------------
 * stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the default stream. */
int maa_ctx_create(int device_id, void* hip_stream, maa_ctx** out);
int maa_ctx_destroy(maa_ctx* ctx);
int maa_ctx_synchronize(maa_ctx* ctx);
int maa_ctx_set_stream(maa_ctx* ctx, void* hip_stream);
/* Arithmetic of the contractions for models CREATED after this call (it fixes their packed weight layout) and
 * for the maa_op_* entry points:
 *   0  exact fp32: v_mfma_f32_32x32x2_f32, bit-for-bit a k-ordered fmaf chain (default)
 *   1  bf16x3: fp32 operands split on the fly into bf16 hi + lo, lo*hi + hi*lo + hi*hi on the bf16 MFMA with fp32
 *      accumulation (~2^-16 per product; meets the fp32 parity gates at 5.3x the fp32 MFMA rate)
 *   2  bf16: operands rounded to bf16, fp32 accumulation (throughput mode, error reported not gated)
 * Storage, normalisations, softmax and every epilogue stay fp32 in all modes. */
int maa_ctx_set_precision(maa_ctx* ctx, int mode);
/* Classifier-free guidance inside maa_ddim_sample (ddim.py:177-199 evaluates the model on cat([x] * 2) in one call): the
 * unconditional and the conditional half of that batch are independent trajectories until the combine, and the library runs
 * them as two lanes -- two branches of the captured step graph, each half on its own stream and workspace -- because one batch
 * of 8 prompts leaves much of the chip idle.  Bit-identical to the one-stream form (every kernel is batch-invariant).
 *   1 two lanes, 0 one stream, -1 the default policy: two lanes unless the caller has said that the chip is kept full from
 * outside (maa_ctx_set_concurrency(ctx, n >= 3) below; measured +4 % for one batch owning the GPU, +3.8 % with two contexts in
 * flight, -24 % with three, profiles/r5/r5_call1_cfg_lanes_ab.txt). */
int maa_ctx_set_cfg_split(maa_ctx* ctx, int mode);
/* The serving arrangement, as a hint (no counterpart in the reference, which runs one request at a time): n = how many contexts'
 * launches the caller keeps in flight on this device.  n >= 3: the chip is kept full from outside, so a launch costs the sum of
 * its workgroups' time rather than the rounds its own grid makes -- a guided DDIM step runs on one stream (as cfg_split 0: six
 * concurrent lanes lose 24 %) and the short-K contractions take the tile with the least total workgroup time (128 x 64 / 128 x 128
 * where one launch alone would take 64 x 64: +0.9 % with three batches in flight, -7 % for a batch alone,
 * profiles/r6_call6_tile_mode_ab.txt).  n = 1 or 2: this context (nearly) owns the GPU -- two CFG lanes (+4 % / +3.8 %), tiles by
 * least launch time.  -1 (default) = not told, treated as 1: a server that keeps three or more batches in flight on as many
 * contexts SHOULD call this (or maa_ctx_set_cfg_split(ctx, 0)) -- left at the default it runs six CFG lanes and loses 24 %.  Every
 * choice is bit-identical; a kept DDIM step graph is dropped when the arrangement changes.  maa_ctx_set_cfg_split overrides the
 * lanes part. */
int maa_ctx_set_concurrency(maa_ctx* ctx, int n);
/* The test / A-B knobs of the environment (MAA_PP, MAA_PP1, MAA_PP_S, MAA_PP_TILE_MAJOR, MAA_UP2, MAA_DMA2, MAA_NO_DMA, MAA_HALO,
 * MAA_OP_PRESPLIT, MAA_GN_TWO_PASS, MAA_EPI) are parsed in one place, when a context is created; this parses them again
 * (and drops the step graph the sampler keeps).  A malformed MAA_DMA2 value fails here (and in maa_ctx_create) with a message
 * naming the variable.  For tests and A/B runs; a -DMAA_NO_TUNING build ignores the environment. */
int maa_ctx_reload_tuning(maa_ctx* ctx);
/* bytes currently reserved for the activation workspace, the second CFG lane's arena included (it exists once a guided sample()
 * has run with two lanes and is kept for the context's lifetime) */
int maa_ctx_workspace_bytes(maa_ctx* ctx, size_t* out);

/* ---- per-kernel timing (replaces the reference's utils.Timer, NeuralSeq/utils/__init__.py:222-237) ----
 * Between begin and end every kernel launch on this context is bracketed by a hipEvent pair on the context's
 * stream; end synchronises and returns one row per kernel (aggregated), with the ALGORITHMIC flops / bytes of
 * the launches.  Launches captured into a hipGraph are not timed (run with use_graph = 0 while profiling). */
typedef struct maa_prof_row {
    char name[48];
    int64_t launches;
    double ms;       /* sum of launch durations */
    double flops;    /* sum of algorithmic flops (2*M*N*K for the contractions) */
    double bytes;    /* sum of algorithmic bytes (compulsory reads + writes) */
} maa_prof_row;
int maa_prof_begin(maa_ctx* ctx, int detail);   /* detail 1: contraction rows are keyed by problem shape */
int maa_prof_end(maa_ctx* ctx, maa_prof_row* rows, int max_rows, int* n_rows);

/* one named fp32 host tensor of a reference state_dict */
typedef struct maa_tensor {
    const char* name;        /* e.g. "input_blocks.1.0.in_layers.2.weight" */
    const float* data;       /* host pointer, contiguous */
    int ndim;
    int64_t shape[6];
} maa_tensor;

/* ---- UNet ---------------------------------------------------------------------------------------
 * Mirrors the constructor arguments of ldm.modules.diffusionmodules.openaimodel.UNetModel
 * (openaimodel.py:443-470) as used by the three shipped configs (txt2audio_args.yaml:31-50,
 * img2audio_args.yaml:31-49, inpaint/txt2audio_args.yaml:30-45). */
typedef struct maa_unet_config {
    int in_channels, out_channels, model_channels;
    int num_res_blocks;
    int n_channel_mult, channel_mult[8];
    int n_attention_resolutions, attention_resolutions[8];
    int num_heads, num_head_channels;          /* -1 = unset, as in the reference */
    int use_spatial_transformer, transformer_depth, context_dim;
    int legacy, resblock_updown;
    int add_context_to_emb;                    /* custom_openaimodel.py:352-354 (I2A) */
} maa_unet_config;

/* replaces: instantiate_from_config(unet_config) + load_state_dict (audio-chatgpt.py:147-152);
 * tensors: the `model.diffusion_model.`-relative entries of the checkpoint */
int maa_unet_create(maa_ctx* ctx, const maa_unet_config* cfg, const maa_tensor* tensors, int n_tensors,
                    maa_unet** out);
int maa_unet_destroy(maa_unet* u);
/* Cross-attention context for the following forwards: d_context [B, L, context_dim] (device).  The K/V
 * projections of every transformer block are computed here, once, and reused by each forward -- the
 * context is constant over a DDIM trajectory (ddim.py:177-198 rebuilds c_in from the same c/uc every step). */
int maa_unet_set_context(maa_ctx* ctx, maa_unet* u, const float* d_context, int B, int L);
/* replaces: UNetModel.forward(x, timesteps, context) (openaimodel.py:711-744 / custom_openaimodel.py:331-368)
 * d_x [B, Cin, H, W], d_t [B] (timesteps as fp32), d_out [B, Cout, H, W].  For the I2A variant the
 * context passed to set_context is also added to the time embedding. */
int maa_unet_forward(maa_ctx* ctx, maa_unet* u, const float* d_x, const float* d_t, int B, int H, int W,
                     float* d_out);

/* replaces: LatentDiffusion_audio.apply_model with `split_input_params` set (ldm/models/diffusion/ddpm_audio.py:572-654;
 * get_fold_unfold :242-293, get_weighting :226-240, delta_border :212-224, meshgrid :205-210): one evaluation of the model on a
 * latent wider than it was trained on.  d_x [B, Cin, H, W] is cut into the L = Ly * Lx crops of kh x kw every sh / sw positions
 * (:250-251; Unfold's order, :582-585), the UNet runs on the B * L crops as one batch with d_t [B] repeated per crop, and
 * d_out [B, Cout, H, W] = fold(eps * weighting) / fold(weighting) (:649-654).  h_weight [kh * kw][L]: the weighting, fp32 on the
 * HOST.  d_context [B, L_tokens, context_dim] with the token count of the last maa_unet_set_context on this UNet (NULL for a UNet
 * without cross-attention): its K/V are projected here, once for the B samples, and served to each sample's crops; afterwards the
 * UNet's context is this one over B * L rows (a plain maa_unet_forward needs maa_unet_set_context again).  (H - kh) % sh == 0,
 * (W - kw) % sw == 0 and stride <= ks are required: the reference divides 0 by 0 at a position no crop covers.  Synchronises the
 * stream once, after the weighting's upload. */
int maa_unet_forward_split(maa_ctx* ctx, maa_unet* u, const float* d_x, const float* d_t, const float* d_context, int B, int H, int W,
                           int kh, int kw, int sh, int sw, const float* h_weight, float* d_out);

/* ---- DDIM ---------------------------------------------------------------------------------------
 * replaces: DDIMSampler.p_sample_ddim's elementwise tail (ddim.py:199, 210-225), eta = 0 or with caller noise:
 *   e = eu + scale*(ec - eu) (ec may be NULL: no guidance);  x0 = (x - sqrt(1-a_t) e)/sqrt(a_t);
 *   x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma^2) e
 * d_coef: device float[4] = {a_t, a_prev, sigma_t, sqrt(1-a_t)} exactly as the sampler's fp32 tables hold them. */
int maa_ddim_update(maa_ctx* ctx, const float* d_x, const float* d_eps_uncond, const float* d_eps_cond, float scale,
                    const float* d_coef, int64_t n, float* d_x_prev, float* d_pred_x0);

/* replaces: DDIMSampler.ddim_sampling (ddim.py:118-166), including mask / x0 blending, eta > 0 with the caller's noise and
 * the logged intermediates (score correctors, quantisation, dropout noise and host callbacks need host code between steps:
 * the Python sampler runs such calls step by step over maa_unet_forward + maa_ddim_update):
 * runs S steps on the device without host round trips.
 *   d_x [B, C, H, W] in/out latent (x_T in, x_0 out)
 *   d_cond / d_uncond [B, L, context_dim] (crossattn; d_uncond NULL or scale == 1 -> no CFG), or for the
 *   concat-conditioned inpaint model d_concat [B, Cc, H, W] (cat([x, c]) -> UNet, ddpm.py:1404-1406)
 *   h_timesteps [S] (ascending DDIM timesteps), h_alphas / h_alphas_prev [S] fp32 tables (host) */
typedef struct maa_ddim_args {
    int S, B, C, H, W;
    float scale;
    const float* d_cond;
    const float* d_uncond;
    int L;
    const float* d_concat;
    int Cc;
    const int32_t* h_timesteps;
    const float* h_alphas;
    const float* h_alphas_prev;
    int use_graph;          /* capture one step into a hipGraph and replay it */
    /* ---- the rest of DDIMSampler.sample's signature (ddim.py:59-115); all optional (NULL / 0) ----
     * mask / x0 (ddim.py:147-150): before every step img = q_sample(x0, t) * mask + (1 - mask) * img, with
     *   q_sample = h_sqrt_ac[i] x0 + h_sqrt_1mac[i] z (ddpm.py:272-275); d_mask, d_x0 [B, C, H, W]; d_noise_q [S][B, C, H, W] =
     *   the S draws of randn_like(x0) in the order the loop makes them (first step first) */
    const float* d_mask;
    const float* d_x0;
    const float* d_noise_q;
    const float* h_sqrt_ac;      /* [S] sqrt(alphas_cumprod[t_i]), sqrt(1 - alphas_cumprod[t_i]) per DDIM index, fp32 as the */
    const float* h_sqrt_1mac;    /*     model's buffers hold them (ddpm.py:139-140) */
    /* eta > 0 (ddim.py:210-225): x_prev += sigma_t * z * temperature; h_sigmas [S] per DDIM index as make_schedule forms them,
     *   d_noise_p [S][B, C, H, W] = the S draws of noise_like(x.shape) in loop order */
    const float* h_sigmas;
    const float* d_noise_p;
    float temperature;
    /* intermediates (ddim.py:158-163): after the step of DDIM index i with i % log_every_t == 0 or i == S - 1 the new latent and
     *   pred_x0 are copied to d_log_x / d_log_x0 [n_log][B, C, H, W], in loop order; n_log must equal the number of such steps */
    int log_every_t;
    int n_log;
    float* d_log_x;
    float* d_log_x0;
    /* split_input_params (LatentDiffusion_audio.apply_model, ldm/models/diffusion/ddpm_audio.py:572-654): every model evaluation
     *   of the loop cuts the latent into crops of split_kh x split_kw every split_sh / split_sw positions (Ly * Lx = L of them,
     *   :250-251), runs the UNet on the B * L crops (2 B * L with guidance) in one batch and stitches its outputs,
     *   sum_l w[p, l] eps_l / sum_l w[p, l] over the crops covering a position.  h_split_weight [split_kh * split_kw][L]: the
     *   reference's weighting (get_weighting, :226-240) as fp32 on the host.  The conditioning's K/V are still projected once per
     *   sample.  All zero / NULL: no split.  Crossattn models only (a concat model with the split fails the call). */
    int split_kh, split_kw, split_sh, split_sw;
    const float* h_split_weight;
} maa_ddim_args;
int maa_ddim_sample(maa_ctx* ctx, maa_unet* u, const maa_ddim_args* args, float* d_x);

/* Text-guided editing (SDEdit): noise an existing latent part of the way, then denoise it under a new prompt.
 * replaces: DDIMSampler.stochastic_encode (ddim.py:227-241):
 *   d_out[b] = h_sqrt_a[t[b]] * x0[b] + h_sqrt_1ma[t[b]] * d_noise[b]      over [B, C, H, W]
 *   d_t [B] device int32, each in [0, n_tab) (checked; an index outside fails the call); h_sqrt_a / h_sqrt_1ma [n_tab] host fp32:
 *   sqrt(ddim_alphas) and ddim_sqrt_one_minus_alphas, or sqrt_alphas_cumprod and sqrt_one_minus_alphas_cumprod (use_original_steps).
 *   from_moments = 0: d_x0_or_moments is x0 [B, C, H, W].  from_moments = 1: it is the VAE moments [B, 2C, H, W] (mean | logvar,
 *   maa_vae_encode_moments) and x0 = scale_factor * (mean + exp(0.5 * clamp(logvar, -30, 20)) * d_noise_post) is formed in the same
 *   pass (DiagonalGaussianDistribution.sample + get_first_stage_encoding).  Synchronises the context's stream. */
int maa_ddim_stochastic_encode(maa_ctx* ctx, const float* d_x0_or_moments, int from_moments, float scale_factor,
                               const float* d_noise_post, const int32_t* d_t, const float* h_sqrt_a, const float* h_sqrt_1ma, int n_tab,
                               const float* d_noise, int B, int C, int H, int W, float* d_out);
/* replaces: DDIMSampler.decode (ddim.py:243-261): args describes the whole S-step schedule as for maa_ddim_sample; the call runs
 * DDIM indices t_start - 1 .. 0 of it on d_x in place (t_start = 0: d_x unchanged; t_start > S: error).  Guidance, concat
 * conditioning and eta > 0 (h_sigmas, d_noise_p [t_start][B, C, H, W] in loop order) as for sample; mask / x0 / logs are rejected.
 * The start index is device state: a decode with the same S, shapes, guidance and buffers as the last sample replays its step graph. */
int maa_ddim_decode(maa_ctx* ctx, maa_unet* u, const maa_ddim_args* args, int t_start, float* d_x);
/* replaces: PLMSSampler.sample / plms_sampling / p_sample_plms (Make-An-Audio ldm/models/diffusion/plms.py:115-236): the
 * pseudo linear multistep trajectory over the S-step schedule args describes, on the device.  Step 0 is the pseudo improved
 * Euler step (two UNet evaluations: eps(x, t) and eps(x_mid, t_next), t_next the next step's timestep, or t itself at the last
 * step); steps 1 .. S-1 are Adams-Bashforth of order min(i, 3) + 1 over the first evaluations of the last three steps (one UNet
 * evaluation each, S + 1 in all).  maa_ddim_args as for maa_ddim_sample (guidance, concat conditioning, mask / x0 before each
 * step's first evaluation, the logs of the final x_prev / pred_x0), except eta: PLMS requires ddim_eta = 0, so h_sigmas and
 * d_noise_p must be NULL (the call fails otherwise) and temperature is ignored.  With use_graph, steps 1 .. S-1 are one captured
 * step replayed, kept on the context apart from maa_ddim_sample's.  (Not the DiffSinger maa_plms_sample below.) */
int maa_ldm_plms_sample(maa_ctx* ctx, maa_unet* u, const maa_ddim_args* args, float* d_x);

/* replaces: LatentDiffusion_audio's own ancestral chain -- p_mean_variance / p_sample / p_sample_loop / progressive_denoising
 * (ldm/models/diffusion/ddpm_audio.py:717-884) -- on the device: the DDPM steps t = start, start - 1, ..., start - n + 1 of the
 * model's num_timesteps-step schedule (p_sample_loop is start = n - 1), one UNet evaluation and one fused kernel each:
 *   e       = eps                                   (eps_u + scale (eps_c - eps_u) with guidance: an extension, the reference's chain has none)
 *   x_recon = h_sqrt_recip_ac[t] x - h_sqrt_recipm1_ac[t] e,  clamped to [-1, 1] when clip_denoised          (ddpm.py:214-218)
 *   mean    = h_coef1[t] x_recon + h_coef2[t] x                                                               (ddpm.py:220-224)
 *   x'      = mean + (t != 0) exp(0.5 h_logvar[t]) (noise_p[v] temperature[t]),  v = start - t                (ddpm_audio.py:766-777)
 *   x'      = (h_sqrt_ac[t] x0 + h_sqrt_1mac[t] noise_q[v]) mask + (1 - mask) x'   with a mask, AFTER the step (ddpm_audio.py:873-875)
 * `loop` carries what the loop shares with maa_ddim_sample: S = num_timesteps (the rows of every table below), B, C, H, W, the
 * conditioning (d_cond / d_uncond / scale / L, or d_concat / Cc), use_graph, d_mask / d_x0 / d_noise_q [n][B, C, H, W], d_noise_p
 * [n][B, C, H, W] (required; both in loop order, first step first), log_every_t / n_log / d_log_x / d_log_x0 and the split.  A step
 * is logged when t % log_every_t == 0 or t == start: x' after the blend -> d_log_x, x_recon after the clamp -> d_log_x0; n_log must
 * equal the number of such steps among the n run.  loop's h_timesteps / h_alphas / h_alphas_prev / h_sqrt_ac / h_sqrt_1mac / h_sigmas /
 * temperature are not read.  The tables are the model's fp32 buffers (ddpm.py:115-155), one row per DDPM timestep, on the host;
 * h_temperature [S] (progressive_denoising's per-timestep list) may be NULL: 1.  The first step runs eagerly and sizes the workspace,
 * then one step is captured and replayed; the graph is kept on the context apart from maa_ddim_sample's and maa_ldm_plms_sample's. */
typedef struct maa_ddpm_args {
    maa_ddim_args loop;
    int start, n;
    int clip_denoised;
    const float* h_sqrt_recip_ac;
    const float* h_sqrt_recipm1_ac;
    const float* h_coef1;
    const float* h_coef2;
    const float* h_logvar;          /* posterior_log_variance_clipped */
    const float* h_sqrt_ac;         /* with a mask: sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod */
    const float* h_sqrt_1mac;
    const float* h_temperature;
} maa_ddpm_args;
int maa_ddpm_sample(maa_ctx* ctx, maa_unet* u, const maa_ddpm_args* args, float* d_x);
/* The same arithmetic for ONE step with a timestep per sample (p_sample, ddpm_audio.py:748-777): d_t [B] device int32 indexes the
 * five host tables of n_tab rows (checked as maa_ddim_stochastic_encode checks its indices); d_eps is the model's output (after any
 * score corrector); d_x_prev = mean + (t != 0) exp(0.5 logvar[t]) (d_noise temperature), d_x_recon = the clamped prediction
 * (return_x0).  Outputs may not alias the inputs.  Synchronises the context's stream. */
int maa_ddpm_update(maa_ctx* ctx, const float* d_x, const float* d_eps, const int32_t* d_t, const float* h_sqrt_recip_ac,
                    const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_logvar, int n_tab,
                    const float* d_noise, float temperature, int clip_denoised, int B, int C, int H, int W, float* d_x_prev,
                    float* d_x_recon);

/* ---- VAE ----------------------------------------------------------------------------------------
 * ddconfig of ldm.models.autoencoder.AutoencoderKL (txt2audio_args.yaml:54-68) */
typedef struct maa_vae_config {
    int ch, out_ch, in_channels, z_channels, embed_dim, resolution, num_res_blocks, double_z;
    int n_ch_mult, ch_mult[8];
    int n_attn_resolutions, attn_resolutions[8];
} maa_vae_config;
/* tensors: the `first_stage_model.`-relative entries (decoder.*, post_quant_conv.*; encoder.*, quant_conv.* optional) */
int maa_vae_create(maa_ctx* ctx, const maa_vae_config* cfg, const maa_tensor* tensors, int n_tensors, maa_vae** out);
int maa_vae_destroy(maa_vae* v);
/* replaces: LatentDiffusion_audio.decode_first_stage (ddpm_audio.py:352-359) -> AutoencoderKL.decode
 * (autoencoder.py:351-354): d_z [B, 4, h, w] -> d_mel [B, out_ch, 8h, 8w]; inv_scale = 1/scale_factor */
int maa_vae_decode(maa_ctx* ctx, maa_vae* v, const float* d_z, int B, int h, int w, float inv_scale, float* d_mel);
/* replaces: decode_first_stage followed by the tools' `torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)` (audio-chatgpt.py:175-176,
 * 254-255, 521-522): d_z [B, 4, h, w] -> d_spec [B, 8h, 8w] in [0, 1], what the vocoders take (one-channel decoders only) */
int maa_vae_decode_spec(maa_ctx* ctx, maa_vae* v, const float* d_z, int B, int h, int w, float inv_scale, float* d_spec);
/* replaces: AutoencoderKL.encode's moments (autoencoder.py:345-349): d_mel [B, 1, H, W] ->
 * d_moments [B, 2*embed_dim, H/8, W/8] = (mean | logvar, unclamped) */
int maa_vae_encode_moments(maa_ctx* ctx, maa_vae* v, const float* d_mel, int B, int H, int W, float* d_moments);

/* ---- vocoder ------------------------------------------------------------------------------------ */
typedef struct maa_vocoder_config {
    int kind;                      /* 0 HiFi-GAN (leaky-ReLU MRF), 1 BigVGAN (anti-aliased snake MRF) */
    int num_mels, upsample_initial_channel;
    int n_upsamples, upsample_rates[8], upsample_kernel_sizes[8];
    int n_kernels, resblock_kernel_sizes[8];
    int n_dilations, resblock_dilation_sizes[8][8];
    int snake_beta, snake_logscale; /* BigVGAN: activation == "snakebeta", snake_logscale */
    /* NSF branch (h['use_pitch_embed'], NeuralSeq/modules/hifigan/hifigan.py:111-115,124-132): harmonic-plus-noise source
     * of `harmonic_num` overtones at `sampling_rate` (h['audio_sample_rate']), added through noise_convs after each ups[i] */
    int use_pitch_embed, sampling_rate, harmonic_num;
    /* h.resblock: 1 (or 0) = ResBlock1 / AMPBlock1 (`convs1` + `convs2`), 2 = ResBlock2 / AMPBlock2 (`convs`: one dilated
     * convolution per residual step; hifigan.py:70-91,119, vocoder/hifigan/modules.py:62-83,93, bigvgan/models.py:90-132,146) */
    int resblock;
} maa_vocoder_config;
/* tensors: generator state_dict (weight_g/weight_v pairs or folded `weight`), keys as
 * NeuralSeq/modules/hifigan/hifigan.py:104-142 / vocoder/bigvgan/models.py:133-179 */
int maa_vocoder_create(maa_ctx* ctx, const maa_vocoder_config* cfg, const maa_tensor* tensors, int n_tensors,
                       maa_vocoder** out);
int maa_vocoder_destroy(maa_vocoder* v);
/* replaces: HifiGanGenerator.forward(x, f0=None) (hifigan.py:144-169), Generator.forward
 * (vocoder/hifigan/modules.py:111-127), BigVGAN.forward (bigvgan/models.py:181-203):
 * d_mel [B, num_mels, T] -> d_wav [B, T*hop] */
int maa_vocoder_forward(maa_ctx* ctx, maa_vocoder* v, const float* d_mel, int B, int T, float* d_wav);
/* replaces: HifiGanGenerator.forward(x, f0) with use_pitch_embed (hifigan.py:144-169: f0_upsamp, m_source, noise_convs)
 * and SineGen / SourceModuleHnNSF (NeuralSeq/modules/parallel_wavegan/models/source.py:399-436, 526-535).
 * d_f0 [B, T] in Hz (0 = unvoiced).  The two random tensors SineGen.forward draws are inputs:
 * d_rand_ini [B, harmonic_num + 1] ~ U[0,1) (initial phase of the overtones; column 0 is ignored) and
 * d_noise [B, T*hop, harmonic_num + 1] ~ N(0,1) (additive noise). */
int maa_vocoder_forward_f0(maa_ctx* ctx, maa_vocoder* v, const float* d_mel, const float* d_f0,
                           const float* d_rand_ini, const float* d_noise, int B, int T, float* d_wav);

/* ---- DiffSinger denoiser + PLMS loop (the singing-voice tool's diffusion hot loop) ---------------
 * DiffNet: NeuralSeq/modules/diff/net.py:84-130 (hparams hidden_size / residual_layers / residual_channels /
 * dilation_cycle_length, in_dims = audio_num_mel_bins) */
typedef struct maa_diffnet_config {
    int in_dims, hidden_size, residual_layers, residual_channels, dilation_cycle_length;
} maa_diffnet_config;
typedef struct maa_diffnet maa_diffnet;
/* tensors: the `denoise_fn.`-relative state_dict of GaussianDiffusion (input_projection.*, mlp.{0,2}.*,
 * residual_layers.{i}.{dilated_conv,diffusion_projection,conditioner_projection,output_projection}.*, skip_projection.*,
 * output_projection.*) */
int maa_diffnet_create(maa_ctx* ctx, const maa_diffnet_config* cfg, const maa_tensor* tensors, int n_tensors,
                       maa_diffnet** out);
int maa_diffnet_destroy(maa_diffnet* d);
/* replaces: DiffNet.forward(spec, diffusion_step, cond) (net.py:107-130):
 * d_spec [B, 1, in_dims, T], d_t [B] (the integer diffusion step as float), d_cond [B, hidden_size, T] -> d_eps [B, 1, in_dims, T] */
int maa_diffnet_forward(maa_ctx* ctx, maa_diffnet* d, const float* d_spec, const float* d_t, const float* d_cond, int B,
                        int T, float* d_eps);
/* replaces: the pndm_speedup branch of GaussianDiffusion.forward(infer=True) (shallow_diffusion_tts.py:262-269) with
 * p_sample_plms (:166-201): t = K_step - interval, ..., 0; d_x [B, 1, in_dims, T] holds x_K on entry and x_0 on return.
 * h_alphas_cumprod [timesteps]: the fp32 buffer of the reference (:82-96). */
typedef struct maa_plms_args {
    int B, T, K_step, interval, timesteps;
    const float* d_cond;              /* [B, hidden_size, T] */
    const float* h_alphas_cumprod;    /* host, [timesteps] */
    int use_graph;
} maa_plms_args;
int maa_plms_sample(maa_ctx* ctx, maa_diffnet* d, const maa_plms_args* args, float* d_x);
/* replaces: the other branch of GaussianDiffusion.forward(infer=True) (shallow_diffusion_tts.py:269-271, hparams['pndm_speedup']
 * unset) and OfflineGaussianDiffusion.forward (:320-321) with p_sample / p_mean_variance / predict_start_from_noise / q_posterior
 * (:134-166): the ancestral steps t = start, start - 1, ..., start - n + 1 of the timesteps-step schedule on d_x
 * [B, 1, in_dims, T] in place (the whole chain: start = K_step - 1, n = K_step), one DiffNet evaluation and one fused kernel each:
 *   x_recon = h_sqrt_recip_ac[t] x - h_sqrt_recipm1_ac[t] eps, clamped to [-1, 1] when clip_denoised
 *   x'      = h_coef1[t] x_recon + h_coef2[t] x + h_sigma[t] noise[start - t]
 * The tables are the reference's fp32 buffers (:111-123), one row per timestep, on the host; h_sigma[t] =
 * exp(0.5 posterior_log_variance_clipped[t]) as p_sample computes it, and row 0 of it is not read: t = 0 adds no noise
 * (nonzero_mask).  d_noise [n][B, 1, in_dims, T]: the call's draws in loop order, first step first (the t = 0 draw is there and
 * is multiplied by zero, as in the reference).  A call equals its consecutive parts bit for bit (start, n1 then start - n1, n - n1).
 * The first step runs eagerly and sizes the workspace, then one step is captured and replayed (use_graph = 0: all eager).
 * in_dims must be a multiple of 4, d_x and d_noise 16-byte aligned, B <= 256. */
typedef struct maa_ds_ddpm_args {
    int B, T, start, n, timesteps;
    int clip_denoised, use_graph;
    const float* d_cond;              /* [B, hidden_size, T] */
    const float* d_noise;             /* [n][B, 1, in_dims, T] */
    const float* h_sqrt_recip_ac;     /* host, [timesteps] each */
    const float* h_sqrt_recipm1_ac;
    const float* h_coef1;
    const float* h_coef2;
    const float* h_sigma;
} maa_ds_ddpm_args;
int maa_ds_ddpm_sample(maa_ctx* ctx, maa_diffnet* d, const maa_ds_ddpm_args* args, float* d_x);
/* The same arithmetic for ONE step with a timestep per sample, after a maa_diffnet_forward (p_sample, :159-166): d_t [B] as the
 * denoiser takes it (the integer step as float) indexes the five host tables of `timesteps` rows; a d_t[b] outside them fails the
 * call.  d_x [B, 1, M, T] in place, d_eps the denoiser's output, d_noise [B, 1, M, T].  Synchronises the context's stream. */
int maa_ds_ddpm_update(maa_ctx* ctx, const float* d_eps, const float* d_t, const float* d_noise, const float* h_sqrt_recip_ac,
                       const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_sigma,
                       int timesteps, int B, int M, int T, int clip_denoised, float* d_x);

/* ---- DiffSinger PitchExtractor (the e2e singing configurations' mel -> f0 between the diffusion and the NSF vocoder) ----
 * NeuralSeq/modules/fastspeech/pe.py:119-149 with hparams hidden_size / predictor_hidden (<= 0: hidden_size) /
 * predictor_kernel / ffn_padding / pitch_type / use_uv / pitch_norm / f0_mean / f0_std (egs_bases/svs/midi/pe.yaml) */
typedef struct maa_pitch_extractor_config {
    int n_mel_bins, hidden_size, predictor_hidden, predictor_kernel, conv_layers;
    int ffn_padding_same;          /* hparams['ffn_padding'] == 'SAME'; anything else is refused */
    int use_uv;                    /* pitch_type == 'frame' and use_uv: frames with a voicing logit > 0 get f0 = 0 */
    int pitch_norm;                /* 0 'log' (f0 = 2 ** x), 1 'standard' (f0 = x * f0_std + f0_mean) */
    float f0_mean, f0_std;
} maa_pitch_extractor_config;
typedef struct maa_pitch_extractor maa_pitch_extractor;
/* tensors: the PitchExtractor state_dict (mel_prenet.layers.{i}.{0,2}.*, mel_prenet.out_proj.*, mel_encoder.{in_proj,out_proj}.*,
 * mel_encoder.conv.{i}.{conv.conv,norm}.*, pitch_predictor.conv.{i}.{1,3}.*, pitch_predictor.linear.*,
 * pitch_predictor.pos_embed_alpha); num_batches_tracked and embed_positions._float_tensor are accepted and ignored */
int maa_pitch_extractor_create(maa_ctx* ctx, const maa_pitch_extractor_config* cfg, const maa_tensor* tensors, int n_tensors,
                               maa_pitch_extractor** out);
int maa_pitch_extractor_destroy(maa_pitch_extractor* pe);
/* replaces: PitchExtractor.forward(mel_input) (pe.py:135-149): d_mel [B, T, n_mel_bins] (a frame of zeros is padding) ->
 * d_pitch_pred [B, T, 2] (ret['pitch_pred']) and d_f0 [B, T] (ret['f0_denorm_pred'], 0 on unvoiced and padding frames).
 * d_mel_hidden: null, or [B, T, hidden_size] receiving pitch_predictor's input.  Launches on the context's stream only. */
int maa_pitch_extractor_forward(maa_ctx* ctx, maa_pitch_extractor* pe, const float* d_mel, int B, int T, float* d_pitch_pred,
                                float* d_f0, float* d_mel_hidden);

/* ---- Glow post-net in reverse (GenerSpeech's and PortaSpeech's last stage: latent + conditioning -> mel) ----
 * NeuralSeq/modules/GenerSpeech/model/glow_modules.py:496-580 Glow.forward(reverse=True) over CouplingBlock, InvConvNear, ActNorm
 * and model/wavenet.py:14-78 WN, as generspeech.py:233-260 run_post_glow calls it; the hparams are post_glow_hidden /
 * post_glow_kernel_size / post_glow_n_blocks / post_glow_n_block_layers / share_wn_layers / sigmoid_scale /
 * post_share_cond_layers (modules/GenerSpeech/config/generspeech.yaml:83-92, egs_bases/tts/ps_flow.yaml).
 * A zero in in_channels, hidden_channels, kernel_size, dilation_rate, n_blocks, n_layers, n_split or n_sqz selects GenerSpeech's
 * shipped value (80, 128, 3, 1, 8, 3, 4, 2); gin_channels, share_cond_layers, share_wn_layers and sigmoid_scale are taken as
 * given (0: no conditioning / false / no sharing).  Refused at creation, with the reason: n_sqz other than 2, n_split other than 4
 * (inv_conv_type 'near' is the one built), an even kernel_size, an odd hidden_channels (and one that is no multiple of 4),
 * in_channels or gin_channels that is no multiple of 4.  p_dropout is not read (eval).  The training direction is not built. */
typedef struct { int in_channels, hidden_channels, kernel_size, dilation_rate, n_blocks, n_layers,
                 n_split, n_sqz, gin_channels, share_cond_layers, share_wn_layers, sigmoid_scale; } maa_glow_config;
typedef struct maa_glow maa_glow;
/* tensors: the Glow state_dict (flows.{3b}.{logs,bias}, flows.{3b+1}.{p,sign_s,l,log_s,u}; its constant buffers l_mask / eye are accepted and not read,
 * flows.{3b+2}.{start,end}.*, flows.{3b+2}.wn.{in_layers,res_skip_layers}.{i}.*, flows.{3b+2}.wn.cond_layer.* or, with
 * share_cond_layers, cond_layer.*); every convolution as the weight-norm pair weight_g / weight_v or as the plain weight that
 * store_inverse leaves.  With share_wn_layers = n the blocks of a group must carry equal in_layers / res_skip_layers.
 * The tensor list is read after the context is bound: with a null context the call fails on the context, whatever the list. */
int maa_glow_create(maa_ctx* ctx, const maa_glow_config* cfg, const maa_tensor* tensors, int n_tensors, maa_glow** out);
int maa_glow_destroy(maa_glow* glow);
/* replaces: Glow.forward(z, x_mask, g=g, reverse=True, return_hiddens=...) in channels-last rows: d_z [B, T, in_channels],
 * d_g [B, T, gin_channels] (null exactly when gin_channels == 0), d_mask [B, T] of 0 / 1 floats (null: all ones) ->
 * d_x [B, 2 (T / 2), in_channels]: an odd last frame is dropped, as the reference's squeeze drops it; a frame pair whose second
 * frame is masked is exact zeros.  d_logdet: null, or [B].  d_hiddens: null, or [3 n_blocks, B, T / 2, 2 in_channels], every
 * flow's output in execution order as squeezed rows (channel s * in_channels + c of row t' is frame 2t' + s).  T < 2 is refused
 * (after the context is bound).  Launches on the context's stream only; two identical calls give the same bits. */
int maa_glow_reverse(maa_ctx* ctx, maa_glow* glow, const float* d_z, const float* d_g, const float* d_mask, int B, int T,
                     float* d_x, float* d_logdet, float* d_hiddens);

/* ---- DiffSinger FastSpeech2MIDI (the e2e singing configurations' front end: score -> decoder_inp, mel2ph, coarse mel) ----
 * NeuralSeq/modules/diffsinger_midi/fs2.py:46-118 over modules/fastspeech/fs2.py:22-72,140-163,222-226 and
 * tts_modules.py:59-143,179-214,276-384, as DiffSingerE2EInfer.forward_model calls it (inference/svs/ds_e2e.py).  The flags
 * below the sizes name hparams whose other values are refused at creation, with the reason. */
typedef struct maa_fs2_config {
    int vocab_size, hidden_size, enc_layers, dec_layers, num_heads;       /* hidden_size / num_heads must be 128 */
    int enc_ffn_kernel_size, dec_ffn_kernel_size;                         /* odd */
    int dur_predictor_layers, dur_predictor_kernel, predictor_hidden;     /* predictor_hidden <= 0: hidden_size */
    int audio_num_mel_bins;
    int ffn_padding_same, ffn_act_gelu, dur_loss_mse, rel_pos, use_pos_embed, encoder_fft, decoder_fft;      /* must be 1 */
    int use_pitch_embed, use_energy_embed, use_spk_id, use_spk_embed, use_bert;                              /* must be 0 */
    /* appended; all zero is FastSpeech2MIDI as above.  plain = 1: the plain FastSpeech2 of modules/fastspeech/fs2.py (the TTS
     * configurations and the *_ds_beta6 chains): no note features, and rel_pos 0 (sinusoid rows by token count), use_energy_embed,
     * use_spk_id (with num_spk, use_split_spk_id) or use_spk_embed are accepted; predictor_layers / predictor_kernel are the
     * energy predictor's.  use_pitch_embed stays refused: the pitch branch is maa_fs2_pitch. */
    int plain, num_spk, use_split_spk_id, predictor_layers, predictor_kernel;
} maa_fs2_config;
typedef struct maa_fs2 maa_fs2;
/* tensors: the FastSpeech2MIDI state_dict ({encoder,decoder}.layers.{i}.op.{layer_norm1,layer_norm2}.*,
 * .op.self_attn.{in_proj_weight,out_proj.weight}, .op.ffn.{ffn_1,ffn_2}.*, {encoder,decoder}.layer_norm.*, encoder.embed_tokens.weight,
 * decoder.pos_embed_alpha, mel_out.*, dur_predictor.conv.{i}.{1,3}.*, dur_predictor.linear.*, midi_embed.weight, midi_dur_layer.*,
 * is_slur_embed.weight); encoder_embed_tokens.weight (the same tensor) and decoder.embed_positions._float_tensor are accepted and
 * ignored */
/* plain = 1: the FastSpeech2 state_dict -- the same without midi_embed / midi_dur_layer / is_slur_embed, plus, by the flags,
 * spk_embed_proj.weight [num_spk + 1, H] (use_spk_id; spk_embed_dur.weight / spk_embed_f0.weight with use_split_spk_id) or
 * spk_embed_proj.{weight [H, 256], bias} (use_spk_embed), and energy_predictor.conv.{i}.{1,3}.*, energy_predictor.linear.* ([1, C_p],
 * [1]), energy_predictor.pos_embed_alpha, energy_embed.weight [256, H] (use_energy_embed) */
int maa_fs2_create(maa_ctx* ctx, const maa_fs2_config* cfg, const maa_tensor* tensors, int n_tensors, maa_fs2** out);
int maa_fs2_destroy(maa_fs2* fs2);
/* The three calls below issue launches on the context's stream only: no device-to-host copy, no synchronisation.  Integer
 * tensors are int32 on the device; their value ranges are the caller's to check (the kernels clamp an index, they do not report).
 *
 * encode: d_tokens [B, T] (0 = padding), d_pitch_midi [B, T] in [0, 300), d_midi_dur [B, T] or NULL, d_is_slur [B, T] in {0, 1}
 * or NULL -> d_encoder_out [B, T, hidden_size] (0 on padding rows), d_xs [B, T] (the duration predictor's log-domain output,
 * ret['dur']), d_dur [B, T] = clamp(round(exp(xs) - 1), min = 0) (ret['dur_choice']) and d_totals [B], the samples' frame counts:
 * T_mel = max(d_totals) is what the caller reads back to size the outputs of the next two calls. */
int maa_fs2_encode(maa_ctx* ctx, maa_fs2* fs2, const int* d_tokens, const int* d_pitch_midi, const float* d_midi_dur,
                   const int* d_is_slur, int B, int T, float* d_encoder_out, float* d_xs, int* d_dur, int* d_totals);
/* ---- the plain FastSpeech2 (a handle created with plain = 1; modules/fastspeech/fs2.py:84-135,165-172, infer only) ----
 * Call order of FastSpeech2.forward: [maa_fs2_speaker] -> maa_fs2_encode_plain -> maa_fs2_length_regulate -> maa_fs2_decode
 * (d_mel_out NULL) -> [maa_fs2_add_speaker] -> [maa_fs2_pitch_forward_from] -> maa_fs2_finish -> maa_fs2_run_decoder.  All of them
 * issue launches on the context's stream only; the handle's mode is read after the context is bound.
 *
 * encode_plain: replaces FastspeechEncoder.forward (tts_modules.py:352-375; positions = cumsum(tok != 0) * (tok != 0) into the
 * sinusoid table, the embedding scale applied once; with rel_pos RelPositionalEncoding on the scaled embedding) and add_dur on
 * dur_inp = (encoder_out + spk_dur) * src_nonpadding.  d_tokens [B, T] (0 = padding), d_spk_dur [B, hidden_size] or NULL ->
 * outputs as maa_fs2_encode.  Refuses a FastSpeech2MIDI handle; maa_fs2_encode refuses a plain one. */
int maa_fs2_encode_plain(maa_ctx* ctx, maa_fs2* fs2, const int* d_tokens, const float* d_spk_dur, int B, int T, float* d_encoder_out,
                         float* d_xs, int* d_dur, int* d_totals);
/* replaces: fs2.py:96-110.  d_ids int32 [3, B] (speaker, dur and f0 ids in [0, num_spk]; rows 1 and 2 are read with
 * use_split_spk_id only) for a use_spk_id handle, d_vec [B, 256] for a use_spk_embed one; both may be non-NULL, the handle's mode
 * chooses -> d_out [3, B, hidden_size] = spk_embed, spk_embed_dur, spk_embed_f0. */
int maa_fs2_speaker(maa_ctx* ctx, maa_fs2* fs2, const int* d_ids, const float* d_vec, int B, float* d_out);
/* d_out [B, T_mel, hidden_size] = (d_x + d_spk[b]) * (mel2ph > 0): pitch_inp, the pitch and energy predictors' input (fs2.py:125) */
int maa_fs2_add_speaker(maa_ctx* ctx, maa_fs2* fs2, const float* d_x, const float* d_spk, const int* d_mel2ph, int B, int T_mel,
                        float* d_out);
/* replaces: add_energy and fs2.py:132.  With use_energy_embed: EnergyPredictor on d_pred_inp [B, T_mel, hidden_size] -> d_energy_pred
 * [B, T_mel] (ret['energy_pred'], every frame); e = d_energy [B, T_mel] if given, else the prediction; bin = floor(64 e) clamped to
 * [0, 255] -> d_energy_bin int32 [B, T_mel].  The reference computes clamp(e * 256 // 4, max = 255) and raises IndexError for a
 * negative e on any frame; here such a frame (and a NaN) takes row 0.  Then, one launch with the head,
 * d_decoder_inp = (d_acc + energy_embed[bin] + d_spk[b]) * (mel2ph > 0) (ret['decoder_inp']; may not alias an input).  d_acc: decode's
 * decoder_inp, or the pitch branch's.  Without use_energy_embed: (d_acc + d_spk[b]) * (mel2ph > 0), d_pred_inp / d_energy unread and
 * d_energy_pred / d_energy_bin unwritten.  d_pred_inp (then), d_energy, d_spk [B, hidden_size], d_energy_pred, d_energy_bin: NULL or given. */
int maa_fs2_finish(maa_ctx* ctx, maa_fs2* fs2, const float* d_pred_inp, const float* d_acc, const int* d_mel2ph, const float* d_energy,
                   const float* d_spk, int B, int T_mel, float* d_decoder_inp, float* d_energy_pred, int* d_energy_bin);
/* LengthRegulator: d_dur [B, T] (>= 0) -> d_mel2ph [B, T_mel], frame -> 1-based token, 0 past the sample's total. */
int maa_fs2_length_regulate(maa_ctx* ctx, maa_fs2* fs2, const int* d_dur, int B, int T, int T_mel, int* d_mel2ph);
/* decode: d_encoder_out [B, T, hidden_size], d_mel2ph [B, T_mel] in [0, T] -> d_decoder_inp [B, T_mel, hidden_size]
 * (ret['decoder_inp']) and, unless NULL (skip_decoder), d_mel_out [B, T_mel, audio_num_mel_bins] (ret['mel_out']); both 0
 * where mel2ph is 0. */
int maa_fs2_decode(maa_ctx* ctx, maa_fs2* fs2, const float* d_encoder_out, const int* d_mel2ph, int B, int T, int T_mel,
                   float* d_decoder_inp, float* d_mel_out);
/* replaces: FastSpeech2.run_decoder (fs2.py:222-226), the second half of decode on a decoder_inp the caller supplies (the pitch
 * branch below finishes one): d_decoder_inp [B, T_mel, hidden_size] (an all-zero row is padding), d_mel2ph [B, T_mel] ->
 * d_mel_out [B, T_mel, audio_num_mel_bins], 0 where mel2ph is 0.  Launches on the context's stream only. */
int maa_fs2_run_decoder(maa_ctx* ctx, maa_fs2* fs2, const float* d_decoder_inp, const int* d_mel2ph, int B, int T_mel,
                        float* d_mel_out);

/* ---- FastSpeech2MIDI pitch branch (the cascade singing configurations: use_pitch_embed over midi/cascade/opencs/aux_rel.yaml) ----
 * FastSpeech2.add_pitch, pitch_type 'frame' (modules/fastspeech/fs2.py:56-64,125-132,187-220): PitchPredictor on the expanded
 * encoder states, denorm_f0, f0_to_coarse (utils/pitch_utils.py:15-31), the pitch_embed row added to decoder_inp.  A second
 * handle beside maa_fs2, which keeps refusing use_pitch_embed: encode -> length_regulate -> decode (d_mel_out NULL) ->
 * maa_fs2_pitch_forward -> maa_fs2_run_decoder. */
typedef struct maa_fs2_pitch_config {
    int hidden_size, predictor_hidden, predictor_layers, predictor_kernel;      /* predictor_hidden <= 0: hidden_size; kernel odd */
    int ffn_padding_same, pitch_type_frame;      /* must be 1: 'LEFT' padding, pitch_type 'ph' and 'cwt' are refused */
    int pitch_ar;                                /* must be 0 */
    int use_uv;                                  /* frames with a voicing logit (or a caller's uv) > 0 get f0 = 0 */
    int pitch_norm;                              /* 0 'log' (f0 = 2 ** x), 1 'standard' (f0 = x * f0_std + f0_mean) */
    float f0_mean, f0_std;
} maa_fs2_pitch_config;
typedef struct maa_fs2_pitch maa_fs2_pitch;
/* tensors: pitch_embed.weight [300, hidden_size], pitch_predictor.conv.{i}.{1,3}.*, pitch_predictor.linear.* ([2, C_p], [2]),
 * pitch_predictor.pos_embed_alpha; pitch_predictor.embed_positions._float_tensor is accepted and ignored, as is every other key
 * of the FastSpeech2MIDI state_dict */
int maa_fs2_pitch_create(maa_ctx* ctx, const maa_fs2_pitch_config* cfg, const maa_tensor* tensors, int n_tensors, maa_fs2_pitch** out);
int maa_fs2_pitch_destroy(maa_fs2_pitch* h);
/* d_origin [B, T_mel, hidden_size]: maa_fs2_decode's d_decoder_inp (decoder_inp_origin; its rows are 0 where mel2ph is 0, which is
 * pitch_inp = origin * (mel2ph > 0) already), d_mel2ph [B, T_mel], d_f0 / d_uv [B, T_mel] or NULL each (the caller's normalised
 * f0 and its unvoiced flags; what is NULL is predicted, and neither is written; without use_uv no frame is unvoiced and d_uv is
 * not read, as denorm_f0 reads uv under hparams['use_uv'] only) -> d_decoder_inp [B, T_mel, hidden_size] =
 * (origin + pitch_embed[coarse]) * (mel2ph > 0) (ret['decoder_inp'], may not alias d_origin), d_pitch_pred [B, T_mel, 2]
 * (ret['pitch_pred']: value and voicing logit; the value is 0 on padding frames when f0 was predicted, as the reference's in-place
 * f0[pitch_padding] = 0 leaves it), d_f0_denorm [B, T_mel] (ret['f0_denorm'], 0 on unvoiced and padding frames) and, unless
 * NULL, d_coarse int32 [B, T_mel], the table rows taken, in [1, 255].  Launches on the context's stream only: no device-to-host
 * copy, no synchronisation. */
int maa_fs2_pitch_forward(maa_ctx* ctx, maa_fs2_pitch* h, const float* d_origin, const int* d_mel2ph, const float* d_f0,
                          const float* d_uv, int B, int T_mel, float* d_decoder_inp, float* d_pitch_pred, float* d_f0_denorm,
                          int* d_coarse);
/* maa_fs2_pitch_forward with the predictor's input d_pred_inp [B, T_mel, hidden_size] -- pitch_inp = (origin + spk_f0) * tgt of a
 * model with speakers (maa_fs2_add_speaker) -- apart from d_origin, which the pitch_embed row is added to.  maa_fs2_pitch_forward
 * is this call with both equal.  d_decoder_inp may alias neither. */
int maa_fs2_pitch_forward_from(maa_ctx* ctx, maa_fs2_pitch* h, const float* d_pred_inp, const float* d_origin, const int* d_mel2ph,
                               const float* d_f0, const float* d_uv, int B, int T_mel, float* d_decoder_inp, float* d_pitch_pred,
                               float* d_f0_denorm, int* d_coarse);

/* ---- conditioning encoders (the step before the sampler: text / image -> cross-attention context) ----------
 * kind 0: the CLAP text branch as FrozenCLAPEmbedder.encode runs it (ldm/modules/encoders/modules.py:204-211):
 *   transformers BertModel (bert-base-uncased, built by TextEncoder, CLAP/clap.py:41-45) on input_ids alone -- no
 *   attention mask, token type 0 -- then Projection (CLAP/clap.py:8-20) on EVERY token: [B, L] ids -> [B, L, d_proj].
 *   tensors: `caption_encoder.`-relative keys: base.embeddings.{word,position,token_type}_embeddings.weight,
 *   base.embeddings.LayerNorm.*, base.encoder.layer.{i}.attention.self.{query,key,value}.*,
 *   .attention.output.{dense,LayerNorm}.*, .intermediate.dense.*, .output.{dense,LayerNorm}.*,
 *   projection.{linear1,linear2}.weight, projection.layer_norm.*
 * kind 1: the OpenCLIP image tower behind FrozenGlobalNormOpenCLIPEmbedder.forward_img (modules.py:340-343):
 *   open_clip VisionTransformer (ViT-H-14: patch 14, width 1280, 32 layers, 16 heads, mlp 5120, GELU), CLS token ->
 *   ln_post -> @ proj, then z / ||z||: [B, 3, image, image] (already preprocessed) -> [B, d_proj].
 *   tensors: `model.visual.`-relative open_clip keys: conv1.weight, class_embedding, positional_embedding, ln_pre.*,
 *   transformer.resblocks.{i}.{ln_1,ln_2}.*, .attn.{in_proj_weight,in_proj_bias}, .attn.out_proj.*, .mlp.{c_fc,c_proj}.*,
 *   ln_post.*, proj ([width, d_proj])
 * kind 2: the OpenCLIP text tower behind FrozenGlobalNormOpenCLIPEmbedder.forward (modules.py:334-338; the image-to-audio
 *   tool encodes its unconditional prompt "" with it, audio-chatgpt.py:238): open_clip CLIP.encode_text (token +
 *   positional embedding, pre-LayerNorm blocks under a causal mask, ln_final, features at the end-of-text token = argmax
 *   of the ids, @ text_projection), then z / ||z||: [B, L] ids -> [B, d_proj].
 *   tensors: `model.`-relative open_clip keys: token_embedding.weight, positional_embedding, transformer.resblocks.{i}.*
 *   (as kind 1), ln_final.*, text_projection ([width, d_proj]) */
typedef struct maa_encoder_config {
    int kind;                       /* 0 = BERT text + CLAP projection, 1 = OpenCLIP ViT image tower, 2 = OpenCLIP text tower */
    int layers, width, heads, mlp_dim, d_proj;
    int vocab, max_positions;       /* kinds 0 and 2 */
    int patch, image;               /* kind 1 */
    float ln_eps;                   /* 1e-12 (BERT) / 1e-5 (ViT) */
} maa_encoder_config;
typedef struct maa_encoder maa_encoder;
int maa_encoder_create(maa_ctx* ctx, const maa_encoder_config* cfg, const maa_tensor* tensors, int n_tensors,
                       maa_encoder** out);
int maa_encoder_destroy(maa_encoder* e);
/* d_ids [B, L] int32 token ids on the device (tokenisation stays on the host);
 * kind 0 -> d_out [B, L, d_proj];  kind 2 -> d_out [B, d_proj], rows L2-normalised */
int maa_encoder_text(maa_ctx* ctx, maa_encoder* e, const int* d_ids, int B, int L, float* d_out);
/* kind 1: d_img [B, 3, image, image] -> d_out [B, d_proj], rows L2-normalised */
int maa_encoder_image(maa_ctx* ctx, maa_encoder* e, const float* d_img, int B, float* d_out);

/* kind 0 only: the scorer's text side -- TextEncoder.forward (wav_evaluation/models/clap.py:49-53: BERT, the [CLS] row,
 * Projection) followed by CLAPWrapper.get_text_embeddings' normalisation (CLAPWrapper.py:177-182).  d_ids holds the
 * UNPADDED token ids: the reference pads to text_len and passes the attention mask, under which the padded keys weigh
 * exactly zero, so the [CLS] row is the same.  -> d_out [B, d_proj], rows L2-normalised */
int maa_encoder_text_cls(maa_ctx* ctx, maa_encoder* e, const int* d_ids, int B, int L, float* d_out);

/* ---- CLAP best-of-n scorer, audio side (T2A.select_best_audio, audio-chatgpt.py:185-199) -------------------
 * replaces: AudioEncoder.forward (wav_evaluation/models/clap.py:22-39) from the log-mel on -- Cnn14.forward after its two
 * extractors (wav_evaluation/models/audio.py:150-176, eval mode) + Projection -- and CLAPWrapper.get_audio_embeddings'
 * normalisation (CLAPWrapper.py:184-189).
 * tensors: `audio_encoder.`-relative keys: base.bn0.*, base.conv_block{1..n}.{conv1,conv2}.weight,
 * base.conv_block{i}.{bn1,bn2}.{weight,bias,running_mean,running_var}, base.fc1.*, projection.{linear1,linear2}.weight,
 * projection.layer_norm.* (fc_audioset and the extractors' frozen tables are not used here) */
typedef struct maa_clap_audio_config {
    int mel_bins, n_blocks, channels[8];
    int out_emb, d_proj;
    float bn_eps;                   /* 1e-5 (nn.BatchNorm2d default) */
} maa_clap_audio_config;
typedef struct maa_clap_audio maa_clap_audio;
int maa_clap_audio_create(maa_ctx* ctx, const maa_clap_audio_config* cfg, const maa_tensor* tensors, int n_tensors,
                          maa_clap_audio** out);
int maa_clap_audio_destroy(maa_clap_audio* a);
/* d_logmel [B, 1, T, mel_bins] -> d_z [B, d_proj] (unit length); d_embedding [B, out_emb] = relu(fc1(.)) or NULL */
int maa_clap_audio_embed(maa_ctx* ctx, maa_clap_audio* a, const float* d_logmel, int B, int T, float* d_embedding,
                         float* d_z);
/* replaces: CLAPWrapper.compute_similarity (CLAPWrapper.py:207-215): d_out [Na, Nt] = scale * audio @ text^T
 * (scale = 1 for use_logit_scale = False, exp(logit_scale) otherwise) */
int maa_clap_similarity(maa_ctx* ctx, const float* d_audio, const float* d_text, int Na, int Nt, int D, float scale,
                        float* d_out);

/* ---- log-mel front ends ------------------------------------------------------------------------------------
 * replaces: torchlibrosa Spectrogram + LogmelFilterBank as Cnn14 builds them (wav_evaluation/models/audio.py:123-131)
 * and TRANSFORMS_16000 (ldm/data/extract_mel_spectrogram.py:15-38, 140-150; Inpaint.gen_mel_audio, audio-chatgpt.py:468-491):
 * centre padding (n_fft / 2 on both sides) -> framed DFT -> re^2 + im^2 (power 2) or its root (power 1) -> mel filter
 * bank -> logarithm.  frames = 1 + n / hop.
 *   h_basis [2 n_freq][n_fft]: rows 0..n_freq-1 the real, n_freq.. the imaginary DFT rows, analysis window folded in
 *     (= torchlibrosa's stft.conv_real.weight / conv_imag.weight, which a CLAP checkpoint carries)
 *   h_melw  [n_mels][n_freq]: the mel filter bank (librosa.filters.mel; = logmel_extractor.melW transposed)
 *   log_kind 0: 10 log10(max(amin, x)) - 10 log10(max(amin, ref))     (power_to_db, top_db = None)
 *   log_kind 1: clip((20 log10(max(amin, x)) - 20 + 100) / 100, 0, 1)  (TRANSFORMS_16000)
 *   out_layout 0: d_out [B, frames, n_mels] (= Cnn14's [B, 1, T, mel_bins]);  1: [B, n_mels, frames] (the LDM's mel image)
 * Always exact fp32, whatever the context's precision mode. */
typedef struct maa_spectral_config {
    int n_fft, hop, n_freq, n_mels;
    int pad_mode;                   /* 0 zeros (librosa >= 0.10), 1 reflect (torchlibrosa; librosa <= 0.9.2) */
    int power;                      /* 1 or 2 */
    int log_kind;
    float amin, ref;
    int out_layout;
} maa_spectral_config;
typedef struct maa_spectral maa_spectral;
int maa_spectral_create(maa_ctx* ctx, const maa_spectral_config* cfg, const float* h_basis, const float* h_melw,
                        maa_spectral** out);
int maa_spectral_destroy(maa_spectral* s);
int maa_spectral_forward(maa_ctx* ctx, maa_spectral* s, const float* d_wav, int B, int n, float* d_out);

/* replaces: torchaudio.transforms.Resample(orig, new) as CLAPWrapper.resample_and_duration applies it
 * (CLAPWrapper.py:103-110): orig / new already divided by their gcd; h_kernels [new][klen], klen = 2 width + orig is
 * torchaudio's sinc kernel bank (built on the host: audiogpt_amd/clap.py).  d_wav [B, n] -> d_out [B, ceil(new n / orig)] */
typedef struct maa_resampler maa_resampler;
int maa_resampler_create(maa_ctx* ctx, int orig, int neu, int width, int klen, const float* h_kernels, maa_resampler** out);
int maa_resampler_destroy(maa_resampler* r);
int maa_resampler_forward(maa_ctx* ctx, maa_resampler* r, const float* d_wav, int B, int n, float* d_out);

/* Box calibration for the benchmark's `box.calib` record (no counterpart in the reference): kind 0 = a fixed register-only
 * loop of dense bf16 MFMAs -> TFLOP/s the box sustains, kind 1 = a fixed 256 MiB device copy -> GB/s (read + written), kind 2 =
 * every workgroup re-reading its own 64 KiB (out of L2) -> GB/s, kind 3 = a 128 MiB buffer re-read by the whole grid (past L2,
 * inside the Infinity Cache) -> GB/s.  Timed with HIP events on the context's stream. */
int maa_calib(maa_ctx* ctx, int kind, double* out_value);

/* ---- single-operator entry points (parity tests and profiling of individual kernels) ------------ */
/* y[M,N] = A[M,K] * W^T (+bias) with W given as torch Linear weight [N,K] on the HOST; A, y on device.
 * The epilogue's other operands, as the models use them (null / 0 = absent): d_res [M,N] is added to the result;
 * c_split != 0 writes y as split32 rows ([32 bf16 hi | 32 bf16 lo] per 32 columns, N % 32 == 0). */
int maa_op_linear(maa_ctx* ctx, const float* d_a, int M, int K, const float* h_w, const float* h_bias, int N,
                  int geglu, float* d_y, const float* d_res, int c_split);
/* conv on channels-first tensors: d_x [B,Cin,H,W] (1-D: H = 1), torch weight [Cout,Cin,KH,KW] on the HOST.
 * d_rowadd [B,Cout] (a ResBlock's time-embedding row) and d_res [B,Cout,Ho,Wo] are added to the result; c_split != 0 leaves
 * the result channels-last, d_y = [B Ho Wo][Cout] split32 rows (Cout % 32 == 0). */
int maa_op_conv(maa_ctx* ctx, const float* d_x, int B, int Cin, int H, int W, const float* h_w, const float* h_bias,
                int Cout, int KH, int KW, int stride, int pad, int dil, int upsample2, float leaky_slope,
                float* d_y, int Ho, int Wo, const float* d_rowadd, const float* d_res, int c_split);
/* GroupNorm(32 groups)(+SiLU) on d_x [B,C,HW] */
int maa_op_groupnorm(maa_ctx* ctx, const float* d_x, int B, int C, int HW, const float* h_gamma,
                     const float* h_beta, float eps, int silu, float* d_y);
/* LayerNorm over the last dim of d_x [rows, C] */
int maa_op_layernorm(maa_ctx* ctx, const float* d_x, int rows, int C, const float* h_gamma, const float* h_beta,
                     float eps, float* d_y);
/* softmax(alpha * q k^T) v per head; q [B,Nq,heads*dh], k/v [B,Nk,heads*dh] -> y [B,Nq,heads*dh] */
int maa_op_attention(maa_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int heads, int dh,
                     int Nq, int Nk, float alpha, float* d_y);
/* The same operator with every argument of the library's internal attention call (tests of the models' layouts):
 * rows of q [B,Nq,*] / k, v [B,Nk,*] have pitch ld{q,k,v} floats and head h starts at column h*hs{q,k,v} of its
 * row; y [B,Nq,*] has pitch ldo >= heads*dh and holds heads*dh dense columns.  out_split = 1 writes y as split32
 * rows (per 32 columns: 32 bf16 high halves, then 32 bf16 low halves; only where the fused kernel runs, an error
 * elsewhere); causal = 1: query i sees keys 0 .. i (Nq == Nk, an error otherwise). */
int maa_op_attention_ex(maa_ctx* ctx, const float* d_q, int ldq, int hsq, const float* d_k, int ldk, int hsk,
                        const float* d_v, int ldv, int hsv, int B, int heads, int dh, int Nq, int Nk, float alpha,
                        float* d_y, int ldo, int out_split, int causal);
/* The same layout with MultiheadAttention's key_padding_mask: d_key_mask [B, Nk] floats, non-zero = the key is hidden from every
 * query of its sample (weight exactly 0).  A sample whose keys are all hidden is written as zeros.  The fused kernel takes
 * dh = 128 in the bf16 modes; every other case runs the three-launch path.  causal must be 0 with a mask (an error otherwise). */
int maa_op_attention_masked(maa_ctx* ctx, const float* d_q, int ldq, int hsq, const float* d_k, int ldk, int hsk,
                            const float* d_v, int ldv, int hsv, int B, int heads, int dh, int Nq, int Nk, float alpha,
                            float* d_y, int ldo, int out_split, int causal, const float* d_key_mask);
/* GroupNorm exactly as the models call it (tests of the normalisation kernels), on channels-last DEVICE buffers the caller has
 * laid out: rows of d_x1 [B,HW,*] have pitch ld1 >= C1 floats and hold channels 0 .. C1; the optional second source d_x2
 * [B,HW,*] (pitch ld2 >= C2; NULL with C2 = 0 for none) holds channels C1 .. C1+C2 -- a decoder ResBlock's (h | skip) without
 * the concatenation.  gamma / beta [C1+C2] on the HOST.  d_y [B,HW,C] is written as the kernels write it: fp32 rows, or split32
 * rows with out_split = 1 (per 32 channels: 32 bf16 high halves, then 32 bf16 low halves; C % 32 == 0).  d_raw (or NULL)
 * [B,HW,C] receives the un-normalised rows in the split32 form.  No layout kernels run in between. */
int maa_op_groupnorm_ex(maa_ctx* ctx, const float* d_x1, int ld1, int C1, const float* d_x2, int ld2, int C2, int B, int HW,
                        int groups, const float* h_gamma, const float* h_beta, float eps, int silu, float* d_y, int out_split,
                        float* d_raw);
/* One contraction exactly as the models issue it (tests of the implicit-GEMM engines and their shared epilogue): the library's
 * internal convolution call, with every field of its descriptor, on channels-last DEVICE buffers the caller has laid out.  No
 * layout kernels run in between and nothing the caller sees is allocated.
 *   A: d_x1 [B,H,W,*] (row pitch ld1 >= C1 floats, channels 0 .. C1) and the optional d_x2 (pitch ld2 >= C2; NULL with C2 = 0)
 *      holding channels C1 .. C1+C2; read through a nearest-2x upsample with up = 1; a_leaky != 0: leaky-relu(a_leaky) of A.
 *      presplit = 1 (bf16 modes, one dense source, C1 % 32 == 0): x1 is first packed into split32 rows, the slope included, the
 *      form the normalisations hand to the LDS-DMA engines.
 *   B: h_w, torch weight [Cout, C1+C2, KH, KW] on the HOST and h_bias [Cout] or NULL, packed as the models pack them; geglu = 1:
 *      h_w [Cout = 2 inner, C1+C2] (KH = KW = 1, bias required) packed value / gate interleaved, the output has N = inner columns.
 *   geometry: stride, dil, pad_w, pad_h (-1: pad_w when KH > 1, else 0); the output is [B,Ho,Wo] positions, taps outside the
 *      source read zero.
 *   epilogue: v = act(alpha * acc + bias + rowadd[b] + res) * out_scale, c = v (+ c with accumulate = 1); d_rowadd [B, *] with
 *      pitch ld_rowadd, d_res pitch ldr, act 0 none / 1 tanh / 2 relu / 3 gelu(erf) / 4 leaky-relu(act_slope); geglu: v = value *
 *      gelu(gate) of (alpha * acc + bias).  d_c [B Ho Wo, *] has pitch ldc >= N and is written as fp32 rows, or with c_split = 1
 *      (N % 32 == 0) as split32 rows; d_c2 (or NULL; N % 32 == 0, pitch ldc2) receives leaky-relu(c, c2_slope) as split32 rows.
 * Checked here: null pointers, positive sizes, the presplit preconditions and pitches no smaller than the widths; everything
 * else is the dispatch's own decision (and error). */
typedef struct {
    const float* d_x1;
    int ld1, C1;
    const float* d_x2;
    int ld2, C2;
    int B, H, W, Ho, Wo;
    const float* h_w;
    const float* h_bias;
    int Cout, KH, KW;
    int stride, pad_w, pad_h, dil, up;
    float a_leaky;
    int presplit;
    float alpha;
    const float* d_rowadd;
    int ld_rowadd;
    const float* d_res;
    int ldr;
    int act;
    float act_slope, out_scale;
    int accumulate, geglu, c_split;
    float* d_c;
    int ldc;
    float* d_c2;
    int ldc2;
    float c2_slope;
} maa_igemm_ex_args;
int maa_op_igemm_ex(maa_ctx* ctx, const maa_igemm_ex_args* args);
/* maa_op_layernorm with the kernels' out_split argument (1: d_y [rows,C] as split32 rows, C % 32 == 0) */
int maa_op_layernorm_ex(maa_ctx* ctx, const float* d_x, int rows, int C, const float* h_gamma, const float* h_beta, float eps,
                        float* d_y, int out_split);
/* One row operator of DiffSinger's sequence models exactly as the models launch it (tests of the one-wave-per-row kernels of
 * pitch.hip / fs2.hip and of the growing sinusoid table): the entry forwards to the library's internal launch and adds no
 * arithmetic.  d_* are DEVICE buffers the caller has laid out, channels-last rows [rows, C]; h_* are HOST arrays, uploaded
 * as the models upload their weights.  C % 4 == 0 everywhere.  kind:
 *   MAA_SEQ_FRAME_MASK   d_x [rows, C] -> d_out [rows] = 0 where every channel of the row is +-0, else 1; d_out2 (or NULL)
 *                        [rows] = 1 - d_out.
 *   MAA_SEQ_AFFINE_MASK  d_out = (d_x * h_scale + h_shift) * d_mask[row], h_scale / h_shift [C] both or neither (neither:
 *                        d_x * d_mask[row]); d_out may be d_x.
 *   MAA_SEQ_GN_RELU_RES  d_out = d_res + relu(GroupNorm(d_x)), d_x / d_res [B * T, C], `groups` groups with the statistics over
 *                        all T frames of a sample, h_gamma / h_beta [C], eps; C / groups a multiple of 4, at most 256; d_out may
 *                        be d_x.
 *   MAA_SEQ_POS_ADD      d_out = d_x + alpha * table[make_positions(d_x[..., 0])], d_x [B, T, C]; the sinusoid table is built
 *                        with table_rows >= 2 rows and grown to T + 1 rows when T + 1 > table_rows, as the models' tables are;
 *                        d_pos (or NULL) int [B, T] receives the positions.
 *   MAA_SEQ_HEAD         a predictor's last LayerNorm (h_gamma / h_beta [C], eps) + Linear(C, n_out) (h_w [n_out, C], h_bias
 *                        [n_out]) on d_x [rows, C], C <= 1024, d_mask [rows].  n_out = 2, the pitch head: d_out [rows, 2] =
 *                        {value, voicing logit}, d_out2 [rows] = denorm_f0 under pitch_norm (0 'log', 1 'standard'), f0_mean,
 *                        f0_std, use_uv, 0 where d_mask is 0.  n_out = 1, the duration head: d_out [rows] = the masked
 *                        prediction xs, d_dur int [rows] = max(rint(exp(xs) - 1), 0).
 * Checked here, before the context is touched: null pointers, rows (B, T) >= 1, C a positive multiple of 4, the head's
 * C <= 1024 and n_out, the GroupNorm channel rule, table_rows >= 2. */
#define MAA_SEQ_FRAME_MASK 0
#define MAA_SEQ_AFFINE_MASK 1
#define MAA_SEQ_GN_RELU_RES 2
#define MAA_SEQ_POS_ADD 3
#define MAA_SEQ_HEAD 4
typedef struct {
    int kind;
    int rows, B, T, C;
    const float* d_x;
    const float* d_res;
    const float* d_mask;
    const float* h_scale;
    const float* h_shift;
    const float* h_gamma;
    const float* h_beta;
    const float* h_w;
    const float* h_bias;
    int groups;
    float eps;
    int table_rows;
    float alpha;
    int n_out, pitch_norm;
    float f0_mean, f0_std;
    int use_uv;
    float* d_out;
    float* d_out2;
    int* d_pos;
    int* d_dur;
} maa_seq_rows_args;
int maa_op_seq_rows(maa_ctx* ctx, const maa_seq_rows_args* args);
/* One row kernel of the Glow post-net run in reverse (csrc/glow.hip) or of the plain FastSpeech2 (csrc/fs2.hip) exactly as the
 * models launch it (tests/test_gpu_tts_ops.py): `kind` selects one internal launch, the entry forwards every argument of it, each
 * nullable pointer included, synchronises the stream once and adds no arithmetic.  d_* are DEVICE buffers the caller has laid
 * out, channels-last rows; h_* are HOST arrays, uploaded as the models upload their weights and tables.  Channel counts are
 * positive multiples of 4.  kind:
 *   MAA_TTS_GLOW_SQUEEZE      d_x [B, T, C] -> d_out [B * (T / 2), 2C]: row t' = [x[2t'], x[2t' + 1]] times d_mask[b, 2t' + 1] (d_mask
 *                             [B, T] or NULL: ones); an odd last frame is not read; d_out2 (or NULL) [B * (T / 2)] receives the
 *                             pairs' mask.  T >= 2.
 *
 *   MAA_TTS_GLOW_GATE         d_x [rows, 2C] -> d_out [rows, C] = tanh(d_x[:, :C]) * sigmoid(d_x[:, C:]).
 *
 *   MAA_TTS_GLOW_WN_RESIDUAL  WN's bookkeeping after one res_skip layer, d_mask [rows], d_out = x [rows, C] and d_out2 = skip
 *                             [rows, C] updated in place.  last = 0: d_x = rs [rows, 2C], x = (x + rs[:, :C]) * mask, skip (+)= rs[:,
 *                             C:].  last = 1: d_x = rs [rows, C], skip = (skip + rs) * mask, x untouched.  first = 1: skip is
 *                             written, not read.
 *
 *   MAA_TTS_GLOW_BLOCK_TAIL   one flow block's tail in reverse on d_x [rows, 2C] with d_y = end(WN(..)) [rows, 2C] = [m | logs] and
 *                             d_mask [rows]: the affine coupling inverse (logs = log(1e-6 + sigmoid(logs + 2)) under
 *                             sigmoid_scale), InvConvNear's 4 x 4 mix with h_winv [16] (row-major [out, in]), ActNorm with h_an_bias
 *                             [2C] and h_an_einv [2C] = exp(-logs) -> d_out [rows, 2C] (may be d_x); d_rowld [rows] (+)= the row's
 *                             share of the coupling's log-determinant (first = 1: written); d_h_cpl / d_h_inv / d_h_act (each
 *                             [rows, 2C] or NULL) receive the three flows' outputs.
 *
 *   MAA_TTS_GLOW_LOGDET       d_out [B] = sum over the sample's T rows of d_x [B, T] + alpha * sum of d_mask [B, T] (alpha: the
 *                             per-frame log-determinant of the mix and ActNorm).
 *
 *   MAA_TTS_FS2_EMBED_PLAIN   forward_embedding of the plain FastSpeech2 as its encode launches it, token positions first: d_tok int
 *                             [B, T], h_table [vocab, C], h_pe [pe_rows, C] (rel = 0: the sinusoid rows, read at the counted
 *                             position, pe_rows > T; rel = 1: RelPositionalEncoding's rows, read at t, pe_rows >= T), alpha = the
 *                             embedding scale -> d_out [B * T, C], d_out2 [B * T] = nonpad, d_out3 [B * T] = 1 - nonpad.
 *
 *   MAA_TTS_FS2_ADD_SPEAKER   d_out [B * T, C] = (d_x + d_spk[b]) * live, d_spk [B, C]; live = d_mask[row] != 0 when d_mask is given,
 *                             else d_mel2ph[row] > 0: exactly one of the two.
 *
 *   MAA_TTS_FS2_SPEAKER_GATHER d_out [3, B, C]: slab k = rows of table k (h_table, h_t1, h_t2, each [n_rows, C]) by d_ids int
 *                             [3, B] (row k with split, row 0 without), clamped into the table; d_ids NULL: row b (n_rows >= B).
 *
 *   MAA_TTS_FS2_ENERGY_TAIL   the end of the variance stage on `rows` frames, T per sample.  With d_x [rows, C], C <= 1024: the
 *                             predictor's last LayerNorm (h_gamma / h_beta [C], eps) + Linear(C, 1) (h_w [C], h_bias [1]) ->
 *                             d_energy_pred (or NULL) [rows]; bin = floor(64 e) in [0, 255] of d_energy (or NULL: of the
 *                             prediction) -> d_bin (or NULL) int [rows]; d_out [rows, H] = (d_y + h_table[bin] + d_spk[b]) *
 *                             (d_mel2ph > 0), h_table [256, H], d_spk [B, H] or NULL.  d_x NULL: d_out = (d_y + d_spk[b]) * (d_mel2ph
 *                             > 0), nothing else is read or written.
 *
 *   MAA_TTS_FS2_TGT_MASK      d_out [rows] = (d_mel2ph[rows] > 0).
 * Checked here, before the context is touched: null pointers per kind, rows (B, T) >= 1, the squeeze's T >= 2, C (and H) positive
 * multiples of 4, the energy head's C <= 1024 and eps, vocab, pe_rows and n_rows against what the kind reads, first / last / rel /
 * split / sigmoid_scale 0 or 1, mask against mel2ph. */
#define MAA_TTS_GLOW_SQUEEZE 0
#define MAA_TTS_GLOW_GATE 1
#define MAA_TTS_GLOW_WN_RESIDUAL 2
#define MAA_TTS_GLOW_BLOCK_TAIL 3
#define MAA_TTS_GLOW_LOGDET 4
#define MAA_TTS_FS2_EMBED_PLAIN 5
#define MAA_TTS_FS2_ADD_SPEAKER 6
#define MAA_TTS_FS2_SPEAKER_GATHER 7
#define MAA_TTS_FS2_ENERGY_TAIL 8
#define MAA_TTS_FS2_TGT_MASK 9
typedef struct {
    int kind;
    int rows, B, T, C, H;
    int first, last, sigmoid_scale, rel, split, vocab, pe_rows, n_rows;
    float eps, alpha;
    const float* d_x;
    const float* d_y;
    const float* d_mask;
    const float* d_spk;
    const float* d_energy;
    const int* d_tok;
    const int* d_mel2ph;
    const int* d_ids;
    const float* h_gamma;
    const float* h_beta;
    const float* h_w;
    const float* h_bias;
    const float* h_table;
    const float* h_t1;
    const float* h_t2;
    const float* h_pe;
    const float* h_winv;
    const float* h_an_bias;
    const float* h_an_einv;
    float* d_out;
    float* d_out2;
    float* d_out3;
    float* d_rowld;
    float* d_h_cpl;
    float* d_h_inv;
    float* d_h_act;
    float* d_energy_pred;
    int* d_bin;
} maa_tts_rows_args;
int maa_op_tts_rows(maa_ctx* ctx, const maa_tts_rows_args* args);
/* One step kernel of the sampling loops exactly as the loops launch it (tests of the ddim_* / ldm_plms_* / ddpm_step and the
 * ds_plms* / ds_ddpm_step kernels of sampler_steps.hip): `kind` selects one internal launch, the entry forwards every argument
 * of it, synchronises the stream once and does nothing else.  EVERY buffer is the caller's DEVICE pointer and is passed through
 * unchanged -- the coefficient slot, the device step index, the tables, the ring, the loop state: no hidden state, no workspace.
 * n = B * per elements of the latent, one sample per `per`; the step's model input d_xin holds nB rows of per_in >= per floats
 * (nB = 2 B: the classifier-free-guidance duplicate, [uncond ; cond]; per_in > per: concat channels behind the latent).  kind:
 *   MAA_STEP_DDIM_PREPARE      idx = *d_step: d_xin [nB, per_in] = cat(d_x [B, per], d_concat [B, per_in - per]) per row (the
 *                              latent first blended with d_mask / d_x0 / draw S - 1 - idx of d_noise_q [S, n] when d_mask),
 *                              d_cur_t [n_t] (n_t <= 0: nB) = d_tab_t[idx], d_coef [8] = row idx of d_tab [S, 8], d_cur_emb
 *                              [emb_w] = row idx of d_emb_tab (or NULL).
 *   MAA_STEP_DDIM              the DDIM update: e = d_eps_u (+ scale (d_eps_c - d_eps_u)), x from the first B rows of d_xin,
 *                              d_coef [8] = {a_t, a_prev, sigma, sqrt(1 - a_t), -, -, log slot, idx}, d_x [n] = x_prev, noise
 *                              sigma z temperature with z = draw S - 1 - idx of d_noise_p (or NULL), slab `log slot` of d_log_x
 *                              / d_log_x0 (slot -1: none), *d_step = idx - 1.
 *   MAA_STEP_PLMS              PLMSSampler's steps i = S - 1 - idx >= 1 over d_ring [3, n]; otherwise as MAA_STEP_DDIM, no noise.
 *   MAA_STEP_PLMS_EULER_MID    its step 0 after the first evaluation: e -> d_e_keep, x -> d_x (the saved latent), x_mid -> the
 *                              latent channels of all nB rows of d_xin, d_cur_t / d_cur_emb to d_tab_t[max(idx - 1, 0)].
 *   MAA_STEP_PLMS_EULER_FINAL  its step 0 after the second evaluation: d_x in place from (d_e_keep + e) / 2, logs, *d_step.
 *   MAA_STEP_DDPM              one ancestral step, t = d_coef[7], row t of d_tab [T, 9] = {sqrt_recip_ac, sqrt_recipm1_ac, coef1,
 *                              coef2, sd, temperature, sqrt_ac, sqrt_1mac, log slot}, draw start - t of d_noise_p and (blend
 *                              after the step, when d_mask) d_noise_q; `clip` clamps x_recon; *d_step = t - 1.
 *   MAA_STEP_DS_PLMS           DiffSinger's PLMS step on d_x [n] with e = d_eps_u, d_tab = alphas_cumprod, d_st = {t, history
 *                              count, ring head}, d_ring [3, n]; mode 0: a multistep step, 1: the predictor into d_x_out (d_x and
 *                              the ring untouched), 2: the corrector with d_e_prev.
 *   MAA_STEP_DS_ADVANCE        d_st = {t - interval, count + 1, (head + 1) % 3}, d_cur_t [B] = max(t - interval, 0); B <= 256.
 *   MAA_STEP_DS_DDPM           DiffSinger's ancestral step on d_x [n] in place, t = d_st[0], row t of d_tab [timesteps, 5], draw
 *                              start - t of d_noise_p [n_steps, n]; n % 4 == 0 and d_x / d_eps_u / d_noise_p 16-byte aligned.
 * Checked here, before the context is touched: null pointers per kind, B, per, n, nB, S, mode, mask without x0 and its noise.
 * The index a kernel reads from a device slot cannot be checked here: the caller keeps it inside its table. */
#define MAA_STEP_DDIM_PREPARE 0
#define MAA_STEP_DDIM 1
#define MAA_STEP_PLMS 2
#define MAA_STEP_PLMS_EULER_MID 3
#define MAA_STEP_PLMS_EULER_FINAL 4
#define MAA_STEP_DDPM 5
#define MAA_STEP_DS_PLMS 6
#define MAA_STEP_DS_ADVANCE 7
#define MAA_STEP_DS_DDPM 8
typedef struct {
    int kind;
    int B, nB, S;
    int64_t n, per, per_in;
    float scale, temperature;
    int start, clip, mode, interval, timesteps, n_steps, emb_w, n_t;
    float* d_x;
    const float* d_concat;
    float* d_xin;
    const float* d_eps_u;
    const float* d_eps_c;
    const float* d_e_prev;
    float* d_coef;
    const float* d_tab_t;
    const float* d_tab;
    int* d_step;
    int* d_st;
    float* d_cur_t;
    const float* d_emb_tab;
    float* d_cur_emb;
    const float* d_mask;
    const float* d_x0;
    const float* d_noise_q;
    const float* d_noise_p;
    float* d_ring;
    float* d_e_keep;
    float* d_x_out;
    float* d_log_x;
    float* d_log_x0;
} maa_sampler_step_args;
int maa_op_sampler_step(maa_ctx* ctx, const maa_sampler_step_args* args);
/* One small kernel of the waveform front ends or of Cnn14's ends exactly as Spectral / Resampler / ClapAudio launch it (tests of
 * csrc/spectral.hip): `kind` selects one internal launch, the entry forwards every argument of it, synchronises the stream once
 * and adds no arithmetic.  d_x / d_out are the caller's DEVICE buffers; h_scale / h_shift are HOST arrays, uploaded as the model
 * uploads its folded BatchNorm.  kind:
 *   MAA_FRONT_PAD     d_x [B, n] -> d_out [B, ldo]: d_out[b, left + i] = d_x[b, i], columns 0 .. left-1 and left+n .. total-1 by
 *                     `mode` (0 zeros, 1 numpy "reflect": needs n > left and n > total - left - n), columns total .. ldo-1 zeros.
 *   MAA_FRONT_POWER   d_x [rows, ldy] = nf real parts then nf imaginary parts per row -> d_out [rows, ldm] = re^2 + im^2
 *                     (power2 != 0) or its square root, columns nf .. ldm-1 zeros.
 *   MAA_FRONT_LOGMEL  d_x [B * frames, ldmel] -> log_kind 0: 10 log10(max(x, amin)) - ref_db; log_kind 1: clip((20 log10(max(x,
 *                     amin)) - 20 + 100) / 100, 0, 1); layout 0: d_out [B, frames, n_mels], 1: d_out [B, n_mels, frames].
 *   MAA_FRONT_AFFINE  d_out [n] = d_x [n] * h_scale[i % F] + h_shift[i % F], h_scale / h_shift [F] (Cnn14.bn0 over the mel bins).
 *   MAA_FRONT_POOL    d_x [B, T, F, C] channels-last -> d_out [B, C] = max_t m + mean_t m, m[t] = mean_f x (Cnn14's pooling).
 * Checked here, before the context is touched: null pointers, every size the kind reads >= 1, left >= 0, total >= left + n,
 * ldo >= total, the reflect rule, ldy >= 2 nf, ldm >= nf, ldmel >= n_mels, amin > 0, kind / mode / log_kind / layout known. */
#define MAA_FRONT_PAD 0
#define MAA_FRONT_POWER 1
#define MAA_FRONT_LOGMEL 2
#define MAA_FRONT_AFFINE 3
#define MAA_FRONT_POOL 4
typedef struct {
    int kind;
    int B, rows, n, T, F, C;
    int left, total, ldo, mode;
    int nf, ldy, ldm, power2;
    int frames, n_mels, ldmel, log_kind, layout;
    float amin, ref_db;
    const float* d_x;
    const float* h_scale;
    const float* h_shift;
    float* d_out;
} maa_front_rows_args;
int maa_op_front_rows(maa_ctx* ctx, const maa_front_rows_args* args);
/* The split32 row codec on its own, d_x / d_y [rows,C] on the device, C % 32 == 0: unpack = 0 writes the split32 rows of
 * leaky_relu(x, slope) (slope 1: of x), unpack = 1 reads split32 rows and writes hi + lo as fp32 (slope is ignored). */
int maa_op_split32(maa_ctx* ctx, const float* d_x, int rows, int C, float slope, int unpack, float* d_y);
/* ConvTranspose1d, d_x [B,Cin,L], torch weight [Cin,Cout,k] on the HOST, padding (k-stride)/2 -> [B,Cout,L*stride].
 * Runs as polyphase GEMMs and refuses what they do not cover: k a multiple of stride, k - stride even, and
 * (stride - 1 + (k - stride) / 2) / stride <= 1 (every k = stride, 2 stride, 3 stride with k - stride even passes). */
int maa_op_conv_transpose1d(maa_ctx* ctx, const float* d_x, int B, int Cin, int L, const float* h_w,
                            const float* h_bias, int Cout, int k, int stride, float leaky_slope, float* d_y);
/* Kernel-only timing of one 3x3 (taps = 9) or 1x1 (taps = 1) convolution [B,H,W,Cin] -> [B,H,W,Cout] in the
 * context's precision mode on synthetic data: `iters` back-to-back launches between two hipEvents.  pre_split = 1
 * feeds the activation as bf16 hi/lo planes (the GroupNorm/LayerNorm output format of the bf16 modes). */
int maa_op_bench_conv(maa_ctx* ctx, int B, int H, int W, int Cin, int Cout, int taps, int pre_split, int iters,
                      float* ms_per_launch);
/* BigVGAN Activation1d (up2 FIR -> snake(beta) -> down2 FIR) on d_x [B,C,L] */
int maa_op_snake_aa(maa_ctx* ctx, const float* d_x, int B, int C, int L, const float* h_alpha, const float* h_beta,
                    int logscale, float* d_y);
/* One residual step of an MRF resblock through the dispatch the generators run (fused pair kernel / halo kernel / implicit
 * GEMM), d_x [B,C,L], torch Conv1d weights [C,C,k] and biases (or NULL) on the HOST, "same" zero padding, odd kernels:
 *   ResBlock1 step:          out = (c2(leaky(c1(leaky(x, slope1)), slope2)) + x) * out_scale
 *   ResBlock2 step (h_w2 NULL): out = (c1(leaky(x, slope1)) + x) * out_scale
 * slope 0 = no activation.  accumulate = 1 adds the result to what d_out [B,C,L] holds; else d_out is overwritten. */
int maa_op_mrf_pair(maa_ctx* ctx, const float* d_x, int B, int C, int L, const float* h_w1, const float* h_b1, int k1, int d1,
                    float slope1, const float* h_w2, const float* h_b2, int k2, int d2, float slope2, float out_scale,
                    int accumulate, float* d_out);
/* The two passes around the UNet of maa_unet_forward_split on their own (ddpm_audio.py:582-585 and :649-654).
 * unfold: d_x [B, C, H, W] -> d_out [B * L, C, kh, kw], row b * L + l the crop l = ly * Lx + lx of sample b: torch.nn.Unfold's
 * columns as images, a copy. */
int maa_op_unfold(maa_ctx* ctx, const float* d_x, int B, int C, int H, int W, int kh, int kw, int sh, int sw, float* d_out);
/* fold: d_crops [B * L, C, kh, kw], h_weight [kh * kw][L] on the HOST -> d_out [B, C, H, W] = (sum_l w[p, l] crop_l[p]) /
 * (sum_l w[p, l]) over the crops that cover a position, in ascending l; the divisor is summed in fp64 and rounded once. */
int maa_op_fold(maa_ctx* ctx, const float* d_crops, const float* h_weight, int B, int C, int H, int W, int kh, int kw, int sh, int sw,
                float* d_out);

#ifdef __cplusplus
}
#endif
#endif /* MAA_H_ */
