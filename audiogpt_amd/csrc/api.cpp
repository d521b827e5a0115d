// extern "C" surface of libaudiogpt_mi355x (include/maa.h): argument checking, handle ownership and the
// exception -> status translation.  No C++ type or exception crosses this file's boundary.
//
// Every entry runs in one order: the argument and configuration checks that touch no device, then bind(ctx), then the work.  A
// malformed call so fails the same way with or without a device, and the checks can be tested without one.  Only a check that
// needs the context's or a model's state comes after bind.  A model handle is made by create_handle and freed by destroy_handle.
#include "models.h"
#include "seq_layers.h"

#include <cstdint>
#include <cstring>
#include <memory>

namespace maa {
const char* last_error_cstr();
}

struct maa_ctx {
    maa::Ctx c;
    bool owns_stream = false;
};
// the opaque handles of maa.h: each owns one model executor
template <class M>
struct Handle {
    using Model = M;
    std::unique_ptr<M> m;
};
struct maa_unet : Handle<maa::UNet> {};
struct maa_vae : Handle<maa::VAE> {};
struct maa_vocoder : Handle<maa::Vocoder> {};
struct maa_diffnet : Handle<maa::DiffNet> {};
struct maa_pitch_extractor : Handle<maa::PitchExtractor> {};
struct maa_glow : Handle<maa::Glow> {};
struct maa_fs2 : Handle<maa::FastSpeech2MIDI> {};
struct maa_fs2_pitch : Handle<maa::FS2Pitch> {};
struct maa_encoder : Handle<maa::Encoder> {};
struct maa_clap_audio : Handle<maa::ClapAudio> {};
struct maa_spectral : Handle<maa::Spectral> {};
struct maa_resampler : Handle<maa::Resampler> {};

namespace {

template <class F>
int guarded(F&& f) {
    try {
        f();
        return MAA_OK;
    } catch (const maa::Error& e) {
        maa::set_last_error(e.what());
        const bool hip = std::strstr(e.what(), "hip") != nullptr;
        return hip ? MAA_ERR_HIP : MAA_ERR_INVALID;
    } catch (const std::exception& e) {
        maa::set_last_error(std::string("internal: ") + e.what());
        return MAA_ERR_INTERNAL;
    } catch (...) {
        maa::set_last_error("internal: unknown exception");
        return MAA_ERR_INTERNAL;
    }
}

maa::StateDict to_state_dict(const maa_tensor* tensors, int n) {
    maa::StateDict sd;
    MAA_CHECK(tensors != nullptr || n == 0, "null tensor list");
    for (int i = 0; i < n; ++i) {
        const maa_tensor& t = tensors[i];
        MAA_CHECK(t.name && t.data && t.ndim >= 0 && t.ndim <= 6, "malformed maa_tensor");
        maa::HostTensor h;
        h.data = t.data;
        for (int d = 0; d < t.ndim; ++d) h.shape.push_back(t.shape[d]);
        sd[t.name] = h;
    }
    return sd;
}

void bind(maa_ctx* ctx) {
    MAA_CHECK(ctx != nullptr, "null context");
    MAA_HIP(hipSetDevice(ctx->c.device));
}

// The handle lifecycle of every model: the executor is constructed into a handle that a unique_ptr owns, and the caller's
// *out receives it only when nothing threw, so a constructor that throws leaves nothing behind.
template <class H, class... Args>
void create_handle(H** out, Args&&... args) {
    auto h = std::make_unique<H>();
    h->m = std::make_unique<typename H::Model>(std::forward<Args>(args)...);
    *out = h.release();
}
template <class H>
int destroy_handle(H* h) {
    return guarded([&] { delete h; });
}

// single-tensor state dict helpers for the operator entry points
struct OneShot {
    maa::StateDict sd;
    void add(const std::string& name, const float* data, std::vector<long long> shape) {
        maa::HostTensor h;
        h.data = data;
        h.shape = std::move(shape);
        sd[name] = h;
    }
};

}  // namespace

extern "C" {

const char* maa_last_error(void) { return maa::last_error_cstr(); }
const char* maa_version(void) { return "libaudiogpt_mi355x 0.1.0 gfx950"; }

int maa_ctx_create(int device_id, void* hip_stream, maa_ctx** out) {
    return guarded([&] {
        MAA_CHECK(out != nullptr, "null out");
        int n = 0;
        MAA_HIP(hipGetDeviceCount(&n));
        MAA_CHECK(device_id >= 0 && device_id < n, "no such HIP device");
        MAA_HIP(hipSetDevice(device_id));
        auto* c = new maa_ctx;
        c->c.device = device_id;
        if (hip_stream) {
            c->c.stream = static_cast<hipStream_t>(hip_stream);
        } else {
            // own stream, created WITHOUT hipStreamNonBlocking: it orders against the legacy default stream
            // (where PyTorch-ROCm puts its copies), and unlike the default stream it can be graph-captured
            hipStream_t s = nullptr;
            hipError_t e = hipStreamCreate(&s);
            if (e != hipSuccess) {
                delete c;
                throw maa::Error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
            }
            c->c.stream = s;
            c->owns_stream = true;
        }
        void* z = nullptr;
        if (hipMalloc(&z, 256) != hipSuccess || hipMemset(z, 0, 256) != hipSuccess) {
            delete c;
            throw maa::Error("hipMalloc: zero page");
        }
        c->c.zeros = static_cast<float*>(z);
        try {
            c->c.tune.load();
        } catch (...) {      // a malformed override: nothing of the half-built context survives the error
            (void)hipFree(z);
            if (c->owns_stream) (void)hipStreamDestroy(c->c.stream);
            delete c;
            throw;
        }
        *out = c;
    });
}
int maa_ctx_destroy(maa_ctx* ctx) {
    return guarded([&] {
        if (!ctx) return;
        (void)hipSetDevice(ctx->c.device);
        (void)hipStreamSynchronize(ctx->c.stream);
        if (ctx->owns_stream) (void)hipStreamDestroy(ctx->c.stream);
        if (ctx->c.zeros) (void)hipFree(ctx->c.zeros);
        delete ctx->c.prof;
        delete ctx;
    });
}
int maa_ctx_reload_tuning(maa_ctx* ctx) {
    return guarded([&] {
        bind(ctx);
        ctx->c.tune.load();
        ctx->c.drop_step_graphs();      // captured under the old knobs
    });
}
int maa_ctx_synchronize(maa_ctx* ctx) {
    return guarded([&] {
        bind(ctx);
        MAA_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}
int maa_ctx_set_stream(maa_ctx* ctx, void* hip_stream) {
    return guarded([&] {
        MAA_CHECK(hip_stream != nullptr, "set_stream needs a non-default stream");
        bind(ctx);
        if (ctx->owns_stream) (void)hipStreamDestroy(ctx->c.stream);
        ctx->owns_stream = false;
        ctx->c.stream = static_cast<hipStream_t>(hip_stream);
    });
}
int maa_ctx_workspace_bytes(maa_ctx* ctx, size_t* out) {
    return guarded([&] {
        MAA_CHECK(out != nullptr, "null argument");
        bind(ctx);
        // the second CFG lane (ddim.cpp) owns a workspace of its own, about half a batch's UNet arena, which is kept once it exists
        *out = ctx->c.ws.capacity() + (ctx->c.side ? ctx->c.side->ws.capacity() : 0);
    });
}

int maa_ctx_set_concurrency(maa_ctx* ctx, int n) {
    return guarded([&] {
        MAA_CHECK(n >= -1 && n != 0, "concurrency: -1 (not told: treated as 1) or the number of contexts kept in flight (>= 1)");
        bind(ctx);
        if (ctx->c.kept_full() != (n >= 3)) ctx->c.drop_step_graphs();      // captured under the other arrangement's launches
        ctx->c.concurrency = n;
    });
}
int maa_ctx_set_cfg_split(maa_ctx* ctx, int mode) {
    return guarded([&] {
        MAA_CHECK(mode >= -1 && mode <= 1, "cfg_split: -1 (default policy), 0 (one stream) or 1 (two lanes)");
        bind(ctx);
        ctx->c.cfg_split = mode;
    });
}

int maa_ctx_set_precision(maa_ctx* ctx, int mode) {
    return guarded([&] {
        MAA_CHECK(mode >= 0 && mode <= 2, "precision mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
        bind(ctx);
        ctx->c.dtype = mode;
    });
}

int maa_prof_begin(maa_ctx* ctx, int detail) {
    return guarded([&] {
        bind(ctx);
        if (!ctx->c.prof) ctx->c.prof = new maa::Profiler;
        ctx->c.prof->detail = detail;
        ctx->c.prof->pending.clear();
        ctx->c.prof->next = 0;
        if (ctx->c.side) {      // (the second lane of a CFG step gets its own table when a step first forks under profiling)
            delete ctx->c.side->prof;
            ctx->c.side->prof = nullptr;
        }
    });
}
int maa_prof_end(maa_ctx* ctx, maa_prof_row* rows, int max_rows, int* n_rows) {
    return guarded([&] {
        MAA_CHECK(rows && n_rows && max_rows > 0, "prof_end without prof_begin / null output");
        bind(ctx);
        MAA_CHECK(ctx->c.prof, "prof_end without prof_begin / null output");
        auto agg = ctx->c.prof->collect(ctx->c.stream);
        delete ctx->c.prof;
        ctx->c.prof = nullptr;
        if (ctx->c.side && ctx->c.side->prof) {      // the launches of the second CFG lane, merged by name
            for (auto& r : ctx->c.side->prof->collect(ctx->c.side->stream)) {
                bool found = false;
                for (auto& a : agg)
                    if (a.name == r.name) {
                        a.launches += r.launches;
                        a.ms += r.ms;
                        a.flops += r.flops;
                        a.bytes += r.bytes;
                        found = true;
                        break;
                    }
                if (!found) agg.push_back(r);
            }
            delete ctx->c.side->prof;
            ctx->c.side->prof = nullptr;
        }
        int n = 0;
        for (auto& r : agg) {
            if (n >= max_rows) break;
            std::memset(&rows[n], 0, sizeof(maa_prof_row));
            std::strncpy(rows[n].name, r.name.c_str(), sizeof(rows[n].name) - 1);
            rows[n].launches = r.launches;
            rows[n].ms = r.ms;
            rows[n].flops = r.flops;
            rows[n].bytes = r.bytes;
            ++n;
        }
        *n_rows = n;
    });
}

// ------------------------------------------------------------------------------------------ UNet
int maa_unet_create(maa_ctx* ctx, const maa_unet_config* cfg, const maa_tensor* tensors, int n_tensors,
                    maa_unet** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out, "null argument");
        MAA_CHECK(cfg->n_channel_mult > 0 && cfg->n_channel_mult <= 8 && cfg->model_channels % 32 == 0,
                  "unsupported UNet config");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_unet_destroy(maa_unet* u) { return destroy_handle(u); }
int maa_unet_set_context(maa_ctx* ctx, maa_unet* u, const float* d_context, int B, int L) {
    return guarded([&] {
        MAA_CHECK(u && d_context && B > 0 && L > 0, "bad set_context arguments");
        bind(ctx);
        u->m->set_context(ctx->c, d_context, B, L);
    });
}
int maa_unet_forward(maa_ctx* ctx, maa_unet* u, const float* d_x, const float* d_t, int B, int H, int W,
                     float* d_out) {
    return guarded([&] {
        MAA_CHECK(u && d_x && d_t && d_out && B > 0 && H > 0 && W > 0, "bad forward arguments");
        bind(ctx);
        u->m->forward(ctx->c, d_x, d_t, u->m->context_ptr, B, H, W, d_out);
    });
}

int maa_unet_forward_split(maa_ctx* ctx, maa_unet* u, const float* d_x, const float* d_t, const float* d_context, int B, int H, int W,
                           int kh, int kw, int sh, int sw, const float* h_weight, float* d_out) {
    return guarded([&] {
        MAA_CHECK(u && d_x && d_t && h_weight && d_out, "bad forward_split arguments: null pointer");
        MAA_CHECK(B > 0, "bad forward_split arguments: empty batch");
        maa::split_check(H, W, kh, kw, sh, sw);
        bind(ctx);
        maa::unet_forward_split(ctx->c, *u->m, d_x, d_t, d_context, B, H, W, kh, kw, sh, sw, h_weight, d_out);
    });
}

int maa_ddim_update(maa_ctx* ctx, const float* d_x, const float* d_eps_uncond, const float* d_eps_cond, float scale,
                    const float* d_coef, int64_t n, float* d_x_prev, float* d_pred_x0) {
    return guarded([&] {
        MAA_CHECK(d_x && d_eps_uncond && d_coef && d_x_prev && n > 0, "bad ddim_update arguments");
        bind(ctx);
        maa::launch_ddim_update(ctx->c, d_x, d_eps_uncond, d_eps_cond, scale, d_coef, n, d_x_prev, d_pred_x0);
    });
}
int maa_ddim_sample(maa_ctx* ctx, maa_unet* u, const maa_ddim_args* args, float* d_x) {
    return guarded([&] {
        MAA_CHECK(u && args && d_x && args->h_timesteps && args->h_alphas && args->h_alphas_prev, "bad ddim_sample arguments");
        bind(ctx);
        maa::ddim_sample(ctx->c, *u->m, *args, d_x);
    });
}
int maa_ddim_stochastic_encode(maa_ctx* ctx, const float* d_x0_or_moments, int from_moments, float scale_factor,
                               const float* d_noise_post, const int32_t* d_t, const float* h_sqrt_a, const float* h_sqrt_1ma, int n_tab,
                               const float* d_noise, int B, int C, int H, int W, float* d_out) {
    return guarded([&] {
        maa::check_stochastic_encode_args(d_x0_or_moments, from_moments != 0, d_noise_post, d_t, h_sqrt_a, h_sqrt_1ma, n_tab, d_noise, B, C,
                                          H, W, d_out);
        bind(ctx);
        maa::ddim_stochastic_encode(ctx->c, d_x0_or_moments, from_moments != 0, scale_factor, d_noise_post, d_t, h_sqrt_a, h_sqrt_1ma,
                                    n_tab, d_noise, B, C, H, W, d_out);
    });
}
int maa_ddim_decode(maa_ctx* ctx, maa_unet* u, const maa_ddim_args* args, int t_start, float* d_x) {
    return guarded([&] {
        maa::check_ddim_decode_args(u, args, t_start, d_x);
        bind(ctx);
        maa::ddim_decode(ctx->c, *u->m, *args, t_start, d_x);
    });
}
int maa_ldm_plms_sample(maa_ctx* ctx, maa_unet* u, const maa_ddim_args* args, float* d_x) {
    return guarded([&] {
        maa::check_ldm_plms_args(u, args, d_x);
        bind(ctx);
        maa::ldm_plms_sample(ctx->c, *u->m, *args, d_x);
    });
}
int maa_ddpm_sample(maa_ctx* ctx, maa_unet* u, const maa_ddpm_args* args, float* d_x) {
    return guarded([&] {
        maa::check_ddpm_sample_args(u, args, d_x);
        bind(ctx);
        maa::ddpm_sample(ctx->c, *u->m, *args, d_x);
    });
}
int maa_ddpm_update(maa_ctx* ctx, const float* d_x, const float* d_eps, const int32_t* d_t, const float* h_sqrt_recip_ac,
                    const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_logvar, int n_tab,
                    const float* d_noise, float temperature, int clip_denoised, int B, int C, int H, int W, float* d_x_prev,
                    float* d_x_recon) {
    return guarded([&] {
        maa::check_ddpm_update_args(d_x, d_eps, d_t, h_sqrt_recip_ac, h_sqrt_recipm1_ac, h_coef1, h_coef2, h_logvar, n_tab, d_noise, B, C, H,
                                    W, d_x_prev, d_x_recon);
        bind(ctx);
        maa::ddpm_update(ctx->c, d_x, d_eps, d_t, h_sqrt_recip_ac, h_sqrt_recipm1_ac, h_coef1, h_coef2, h_logvar, n_tab, d_noise,
                         temperature, clip_denoised != 0, B, C, H, W, d_x_prev, d_x_recon);
    });
}

// ------------------------------------------------------------------------------------------ VAE
int maa_vae_create(maa_ctx* ctx, const maa_vae_config* cfg, const maa_tensor* tensors, int n_tensors, maa_vae** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out && cfg->n_ch_mult > 0 && cfg->n_ch_mult <= 8, "bad VAE config");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_vae_destroy(maa_vae* v) { return destroy_handle(v); }
int maa_vae_decode(maa_ctx* ctx, maa_vae* v, const float* d_z, int B, int h, int w, float inv_scale, float* d_mel) {
    return guarded([&] {
        MAA_CHECK(v && d_z && d_mel && B > 0 && h > 0 && w > 0, "bad vae_decode arguments");
        bind(ctx);
        v->m->decode(ctx->c, d_z, B, h, w, inv_scale, d_mel);
    });
}
int maa_vae_decode_spec(maa_ctx* ctx, maa_vae* v, const float* d_z, int B, int h, int w, float inv_scale, float* d_spec) {
    return guarded([&] {
        MAA_CHECK(v && d_z && d_spec && B > 0 && h > 0 && w > 0, "bad vae_decode_spec arguments");
        bind(ctx);
        v->m->decode_spec(ctx->c, d_z, B, h, w, inv_scale, d_spec);
    });
}
int maa_vae_encode_moments(maa_ctx* ctx, maa_vae* v, const float* d_mel, int B, int H, int W, float* d_moments) {
    return guarded([&] {
        MAA_CHECK(v && d_mel && d_moments && B > 0 && H > 0 && W > 0, "bad vae_encode arguments");
        bind(ctx);
        v->m->encode_moments(ctx->c, d_mel, B, H, W, d_moments);
    });
}

// ------------------------------------------------------------------------------------------ vocoder
int maa_vocoder_create(maa_ctx* ctx, const maa_vocoder_config* cfg, const maa_tensor* tensors, int n_tensors,
                       maa_vocoder** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out && cfg->n_upsamples > 0 && cfg->n_upsamples <= 8 && cfg->n_kernels > 0 &&
                      cfg->n_kernels <= 8 && cfg->n_dilations > 0 && cfg->n_dilations <= 8,
                  "bad vocoder config");
        // (the generator's build refuses these too)
        for (int i = 0; i < cfg->n_upsamples; ++i) maa::check_convtr_polyphase(cfg->upsample_kernel_sizes[i], cfg->upsample_rates[i]);
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_vocoder_destroy(maa_vocoder* v) { return destroy_handle(v); }
int maa_vocoder_forward(maa_ctx* ctx, maa_vocoder* v, const float* d_mel, int B, int T, float* d_wav) {
    return guarded([&] {
        MAA_CHECK(v && d_mel && d_wav && B > 0 && T > 0, "bad vocoder_forward arguments");
        bind(ctx);
        v->m->forward(ctx->c, d_mel, B, T, d_wav);
    });
}
int maa_vocoder_forward_f0(maa_ctx* ctx, maa_vocoder* v, const float* d_mel, const float* d_f0, const float* d_rand_ini,
                           const float* d_noise, int B, int T, float* d_wav) {
    return guarded([&] {
        MAA_CHECK(v && d_mel && d_f0 && d_rand_ini && d_noise && d_wav && B > 0 && T > 0, "bad vocoder_forward_f0 arguments");
        bind(ctx);
        v->m->forward_f0(ctx->c, d_mel, d_f0, d_rand_ini, d_noise, B, T, d_wav);
    });
}

// ------------------------------------------------------------------------------------------ operators
// ------------------------------------------------------------------------------------------ DiffSinger
int maa_diffnet_create(maa_ctx* ctx, const maa_diffnet_config* cfg, const maa_tensor* tensors, int n_tensors,
                       maa_diffnet** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out && cfg->in_dims > 0 && cfg->hidden_size > 0 && cfg->residual_layers > 0 &&
                      cfg->residual_channels > 0 && cfg->residual_channels % 2 == 0 && cfg->dilation_cycle_length > 0,
                  "bad DiffNet config");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_diffnet_destroy(maa_diffnet* d) { return destroy_handle(d); }
int maa_diffnet_forward(maa_ctx* ctx, maa_diffnet* d, const float* d_spec, const float* d_t, const float* d_cond, int B,
                        int T, float* d_eps) {
    return guarded([&] {
        MAA_CHECK(d && d_spec && d_t && d_cond && d_eps && B > 0 && T > 0, "bad diffnet_forward arguments");
        bind(ctx);
        d->m->forward(ctx->c, d_spec, d_t, d_cond, B, T, d_eps);
    });
}
int maa_plms_sample(maa_ctx* ctx, maa_diffnet* d, const maa_plms_args* args, float* d_x) {
    return guarded([&] {
        MAA_CHECK(d && args && d_x, "bad plms_sample arguments");
        bind(ctx);
        d->m->plms_sample(ctx->c, *args, d_x);
    });
}
int maa_ds_ddpm_sample(maa_ctx* ctx, maa_diffnet* d, const maa_ds_ddpm_args* args, float* d_x) {
    return guarded([&] {
        MAA_CHECK(d && args && d_x, "bad ds_ddpm_sample arguments: null pointer");
        bind(ctx);
        d->m->ddpm_sample(ctx->c, *args, d_x);
    });
}
int maa_ds_ddpm_update(maa_ctx* ctx, const float* d_eps, const float* d_t, const float* d_noise, const float* h_sqrt_recip_ac,
                       const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_sigma,
                       int timesteps, int B, int M, int T, int clip_denoised, float* d_x) {
    return guarded([&] {
        MAA_CHECK(d_eps && d_t && d_noise && d_x, "bad ds_ddpm_update arguments: null pointer");
        MAA_CHECK(h_sqrt_recip_ac && h_sqrt_recipm1_ac && h_coef1 && h_coef2 && h_sigma,
                  "bad ds_ddpm_update arguments: the posterior tables are missing");
        MAA_CHECK(d_x != d_eps && d_x != d_noise, "bad ds_ddpm_update arguments: d_x is updated in place and may not alias the inputs");
        bind(ctx);
        maa::ds_ddpm_update(ctx->c, d_eps, d_t, d_noise, h_sqrt_recip_ac, h_sqrt_recipm1_ac, h_coef1, h_coef2, h_sigma, timesteps,
                            B, M, T, clip_denoised != 0, d_x);
    });
}

// ------------------------------------------------------------------------------------------ DiffSinger PitchExtractor
int maa_pitch_extractor_create(maa_ctx* ctx, const maa_pitch_extractor_config* cfg, const maa_tensor* tensors, int n_tensors,
                               maa_pitch_extractor** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out, "bad pitch_extractor_create arguments: null pointer");
        MAA_CHECK(cfg->ffn_padding_same != 0,
                  "PitchExtractor: hparams['ffn_padding'] must be 'SAME' -- the causal 'LEFT' padding (kernel - 1, 0) is not built");
        MAA_CHECK(cfg->n_mel_bins > 0 && cfg->n_mel_bins % 4 == 0 && cfg->hidden_size >= 16 && cfg->hidden_size % 16 == 0 &&
                      cfg->conv_layers >= 0,
                  "bad PitchExtractor config: n_mel_bins must be a multiple of 4, hidden_size a multiple of 16, conv_layers >= 0");
        MAA_CHECK(cfg->predictor_hidden <= 1024 && (cfg->predictor_hidden <= 0 || cfg->predictor_hidden % 4 == 0) &&
                      cfg->hidden_size <= 1024,
                  "bad PitchExtractor config: predictor_hidden must be a multiple of 4 (or <= 0 for hidden_size), widths at most 1024");
        MAA_CHECK(cfg->predictor_kernel >= 1 && cfg->predictor_kernel % 2 == 1,
                  "bad PitchExtractor config: predictor_kernel must be odd ('SAME' padding keeps the length only then)");
        MAA_CHECK(cfg->pitch_norm == 0 || cfg->pitch_norm == 1, "bad PitchExtractor config: pitch_norm is 0 ('log') or 1 ('standard')");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_pitch_extractor_destroy(maa_pitch_extractor* pe) { return destroy_handle(pe); }
int maa_pitch_extractor_forward(maa_ctx* ctx, maa_pitch_extractor* pe, const float* d_mel, int B, int T, float* d_pitch_pred,
                                float* d_f0, float* d_mel_hidden) {
    return guarded([&] {
        MAA_CHECK(pe && d_mel && d_pitch_pred && d_f0, "bad pitch_extractor_forward arguments: null pointer");
        MAA_CHECK(B > 0 && T > 0 && (long long)B * T < (1LL << 31) / 1024, "bad pitch_extractor_forward arguments: B, T");
        bind(ctx);
        pe->m->forward(ctx->c, d_mel, B, T, d_pitch_pred, d_f0, d_mel_hidden);
    });
}

// ------------------------------------------------------------------------------------------ Glow post-net (reverse)
int maa_glow_create(maa_ctx* ctx, const maa_glow_config* cfg, const maa_tensor* tensors, int n_tensors, maa_glow** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out, "bad glow_create arguments: null pointer");
        maa::check_glow_config(*cfg);
        // The one entry that binds before its last argument check: the tensor list is converted (and a null list with
        // n_tensors > 0 refused) only here, after the context.  The entry-order test calls every create entry with a null list of one
        // tensor and expects the null context to be what refuses it.
        bind(ctx);
        auto sd = to_state_dict(tensors, n_tensors);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_glow_destroy(maa_glow* glow) { return destroy_handle(glow); }
int maa_glow_reverse(maa_ctx* ctx, maa_glow* glow, const float* d_z, const float* d_g, const float* d_mask, int B, int T,
                     float* d_x, float* d_logdet, float* d_hiddens) {
    return guarded([&] {
        maa::check_glow_reverse_args(glow, d_z, B, T, d_x);
        bind(ctx);
        // (T < 2 and d_g against the model's gin_channels are refused in the model: they need the handle's state)
        glow->m->reverse(ctx->c, d_z, d_g, d_mask, B, T, d_x, d_logdet, d_hiddens);
    });
}

// ------------------------------------------------------------------------------------------ DiffSinger FastSpeech2MIDI
int maa_fs2_create(maa_ctx* ctx, const maa_fs2_config* cfg, const maa_tensor* tensors, int n_tensors, maa_fs2** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out, "bad fs2_create arguments: null pointer");
        MAA_CHECK(!cfg->use_pitch_embed, "FastSpeech2MIDI: hparams['use_pitch_embed'] is not built into this handle -- the pitch branch is maa_fs2_pitch, beside it");
        if (cfg->plain) {      // the plain FastSpeech2: energy, speakers and the token-counted sinusoid positions live in this handle
            MAA_CHECK(cfg->use_pos_embed != 0, "FastSpeech2: hparams['use_pos_embed'] must be true -- an encoder without positions is not built");
            MAA_CHECK(!(cfg->use_spk_id && cfg->use_spk_embed),
                      "FastSpeech2: hparams['use_spk_id'] and ['use_spk_embed'] are alternatives (fs2.py:41-47) -- set one");
            MAA_CHECK(!cfg->use_spk_id || (cfg->num_spk >= 1 && cfg->num_spk < (1 << 24)),
                      "bad FastSpeech2 config: use_spk_id needs num_spk >= 1 (the table has num_spk + 1 rows)");
            MAA_CHECK(!cfg->use_split_spk_id || cfg->use_spk_id, "bad FastSpeech2 config: use_split_spk_id without use_spk_id");
            MAA_CHECK(!cfg->use_energy_embed || (cfg->predictor_layers >= 1 && cfg->predictor_kernel >= 1 && cfg->predictor_kernel % 2 == 1),
                      "bad FastSpeech2 config: use_energy_embed needs predictor_layers >= 1 and an odd predictor_kernel ('SAME' padding "
                      "keeps the length only then)");
        } else {
            MAA_CHECK(!cfg->use_energy_embed, "FastSpeech2MIDI: hparams['use_energy_embed'] is not built -- no shipped e2e singing configuration sets it");
            MAA_CHECK(!cfg->use_spk_id && !cfg->use_spk_embed,
                      "FastSpeech2MIDI: hparams['use_spk_id'] / ['use_spk_embed'] are not built -- no shipped e2e singing configuration sets them");
        }
        MAA_CHECK(!cfg->use_bert, "FastSpeech2MIDI: hparams['use_bert'] is not built -- no shipped e2e singing configuration sets it");
        MAA_CHECK(cfg->plain || (cfg->rel_pos != 0 && cfg->use_pos_embed != 0),
                  "FastSpeech2MIDI: hparams['rel_pos'] and ['use_pos_embed'] must be true -- only RelPositionalEncoding is built for the encoder");
        MAA_CHECK(cfg->ffn_padding_same != 0,
                  "FastSpeech2MIDI: hparams['ffn_padding'] must be 'SAME' -- the causal 'LEFT' padding (kernel - 1, 0) is not built");
        MAA_CHECK(cfg->ffn_act_gelu != 0, "FastSpeech2MIDI: hparams['ffn_act'] must be 'gelu' -- the only activation built into the FFN's epilogue here");
        MAA_CHECK(cfg->dur_loss_mse != 0, "FastSpeech2MIDI: hparams['dur_loss'] must be 'mse' -- out2dur's other branches are not built");
        MAA_CHECK(cfg->encoder_fft != 0 && cfg->decoder_fft != 0, "FastSpeech2MIDI: hparams['encoder_type'] / ['decoder_type'] must be 'fft'");
        MAA_CHECK(cfg->num_heads > 0 && cfg->hidden_size == 128 * cfg->num_heads,
                  "FastSpeech2MIDI: hidden_size / num_heads must be 128 -- the only head width the masked attention is built and tested for");
        MAA_CHECK(cfg->vocab_size > 0 && cfg->enc_layers >= 0 && cfg->dec_layers >= 0 && cfg->hidden_size <= 1024 &&
                      cfg->audio_num_mel_bins > 0 && cfg->audio_num_mel_bins % 4 == 0,
                  "bad FastSpeech2MIDI config: vocab_size > 0, layer counts >= 0, hidden_size <= 1024, audio_num_mel_bins a multiple of 4");
        MAA_CHECK(cfg->enc_ffn_kernel_size >= 1 && cfg->enc_ffn_kernel_size % 2 == 1 && cfg->dec_ffn_kernel_size >= 1 &&
                      cfg->dec_ffn_kernel_size % 2 == 1 && cfg->dur_predictor_kernel >= 1 && cfg->dur_predictor_kernel % 2 == 1,
                  "bad FastSpeech2MIDI config: the FFN and predictor kernels must be odd ('SAME' padding keeps the length only then)");
        MAA_CHECK(cfg->dur_predictor_layers >= 1 && cfg->predictor_hidden <= 1024 && (cfg->predictor_hidden <= 0 || cfg->predictor_hidden % 4 == 0),
                  "bad FastSpeech2MIDI config: dur_predictor_layers >= 1, predictor_hidden a multiple of 4 (or <= 0 for hidden_size), at most 1024");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_fs2_destroy(maa_fs2* fs2) { return destroy_handle(fs2); }
int maa_fs2_encode(maa_ctx* ctx, maa_fs2* fs2, const int* d_tokens, const int* d_pitch_midi, const float* d_midi_dur,
                   const int* d_is_slur, int B, int T, float* d_encoder_out, float* d_xs, int* d_dur, int* d_totals) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_tokens&& d_pitch_midi && d_encoder_out && d_xs && d_dur && d_totals, "bad fs2_encode arguments: null pointer");
        MAA_CHECK(B > 0 && T > 0 && (long long)B * T < (1LL << 31) / 4096, "bad fs2_encode arguments: B, T");
        bind(ctx);
        fs2->m->encode(ctx->c, d_tokens, d_pitch_midi, d_midi_dur, d_is_slur, B, T, d_encoder_out, d_xs, d_dur, d_totals);
    });
}
int maa_fs2_encode_plain(maa_ctx* ctx, maa_fs2* fs2, const int* d_tokens, const float* d_spk_dur, int B, int T, float* d_encoder_out,
                         float* d_xs, int* d_dur, int* d_totals) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_tokens && d_encoder_out && d_xs && d_dur && d_totals, "bad fs2_encode_plain arguments: null pointer");
        MAA_CHECK(B > 0 && T > 0 && (long long)B * T < (1LL << 31) / 4096, "bad fs2_encode_plain arguments: B, T");
        bind(ctx);
        fs2->m->encode_plain(ctx->c, d_tokens, d_spk_dur, B, T, d_encoder_out, d_xs, d_dur, d_totals);
    });
}
int maa_fs2_speaker(maa_ctx* ctx, maa_fs2* fs2, const int* d_ids, const float* d_vec, int B, float* d_out) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_out, "bad fs2_speaker arguments: null pointer");
        MAA_CHECK(d_ids || d_vec, "bad fs2_speaker arguments: neither d_ids nor d_vec");
        MAA_CHECK(B > 0 && 3LL * B < (1LL << 31) / 4096,"bad fs2_speaker arguments: B");
        bind(ctx);
        fs2->m->speaker(ctx->c, d_ids, d_vec, B, d_out);
    });
}
int maa_fs2_add_speaker(maa_ctx* ctx, maa_fs2* fs2, const float* d_x, const float* d_spk, const int* d_mel2ph, int B, int T_mel,
                        float* d_out) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_x && d_spk && d_mel2ph && d_out, "bad fs2_add_speaker arguments: null pointer");
        MAA_CHECK(B > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_add_speaker arguments: B, T_mel");
        bind(ctx);
        fs2->m->add_speaker(ctx->c, d_x, d_spk, d_mel2ph, B, T_mel, d_out);
    });
}
int maa_fs2_finish(maa_ctx* ctx, maa_fs2* fs2, const float* d_pred_inp, const float* d_acc, const int* d_mel2ph, const float* d_energy,
                   const float* d_spk, int B, int T_mel, float* d_decoder_inp, float* d_energy_pred, int* d_energy_bin) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_acc && d_mel2ph && d_decoder_inp, "bad fs2_finish arguments: null pointer");
        MAA_CHECK(B > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_finish arguments: B, T_mel");
        MAA_CHECK(d_decoder_inp != d_acc && d_decoder_inp != d_pred_inp, "bad fs2_finish arguments: d_decoder_inp may not alias d_acc or d_pred_inp");
        bind(ctx);
        fs2->m->finish(ctx->c, d_pred_inp, d_acc, d_mel2ph, d_energy, d_spk, B, T_mel, d_decoder_inp, d_energy_pred, d_energy_bin);
    });
}
int maa_fs2_length_regulate(maa_ctx* ctx, maa_fs2* fs2, const int* d_dur, int B, int T, int T_mel, int* d_mel2ph) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_dur&& d_mel2ph, "bad fs2_length_regulate arguments: null pointer");
        MAA_CHECK(B > 0 && T > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_length_regulate arguments: B, T, T_mel");
        bind(ctx);
        fs2->m->length_regulate(ctx->c, d_dur, B, T, T_mel, d_mel2ph);
    });
}
int maa_fs2_decode(maa_ctx* ctx, maa_fs2* fs2, const float* d_encoder_out, const int* d_mel2ph, int B, int T, int T_mel,
                   float* d_decoder_inp, float* d_mel_out) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_encoder_out&& d_mel2ph && d_decoder_inp, "bad fs2_decode arguments: null pointer");
        MAA_CHECK(B > 0 && T > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_decode arguments: B, T, T_mel");
        bind(ctx);
        fs2->m->decode(ctx->c, d_encoder_out, d_mel2ph, B, T, T_mel, d_decoder_inp, d_mel_out);
    });
}
int maa_fs2_run_decoder(maa_ctx* ctx, maa_fs2* fs2, const float* d_decoder_inp, const int* d_mel2ph, int B, int T_mel, float* d_mel_out) {
    return guarded([&] {
        MAA_CHECK(fs2 && d_decoder_inp&& d_mel2ph && d_mel_out, "bad fs2_run_decoder arguments: null pointer");
        MAA_CHECK(B > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_run_decoder arguments: B, T_mel");
        bind(ctx);
        fs2->m->run_decoder(ctx->c, d_decoder_inp, d_mel2ph, B, T_mel, d_mel_out);
    });
}

// ------------------------------------------------------------------------------------------ FastSpeech2MIDI pitch branch
int maa_fs2_pitch_create(maa_ctx* ctx, const maa_fs2_pitch_config* cfg, const maa_tensor* tensors, int n_tensors, maa_fs2_pitch** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out, "bad fs2_pitch_create arguments: null pointer");
        MAA_CHECK(cfg->pitch_type_frame != 0,
                  "FastSpeech2MIDI pitch: hparams['pitch_type'] must be 'frame' -- 'ph' is not built, and 'cwt' reads cwt_predictor / "
                  "cwt_stats_layers, which the reference's FastSpeech2 never creates");
        MAA_CHECK(!cfg->pitch_ar, "FastSpeech2MIDI pitch: hparams['pitch_ar'] is not built -- no shipped singing configuration sets it");
        MAA_CHECK(cfg->ffn_padding_same != 0,
                  "FastSpeech2MIDI pitch: hparams['ffn_padding'] must be 'SAME' -- the causal 'LEFT' padding (kernel - 1, 0) is not built");
        MAA_CHECK(cfg->pitch_norm == 0 || cfg->pitch_norm == 1, "bad FastSpeech2MIDI pitch config: pitch_norm is 0 ('log') or 1 ('standard')");
        MAA_CHECK(cfg->hidden_size >= 4 && cfg->hidden_size % 4 == 0 && cfg->hidden_size <= 1024 && cfg->predictor_hidden <= 1024 &&
                      (cfg->predictor_hidden <= 0 || cfg->predictor_hidden % 4 == 0),
                  "bad FastSpeech2MIDI pitch config: hidden_size and predictor_hidden (<= 0 for hidden_size) multiples of 4, at most 1024");
        MAA_CHECK(cfg->predictor_layers >= 1 && cfg->predictor_kernel >= 1 && cfg->predictor_kernel % 2 == 1,
                  "bad FastSpeech2MIDI pitch config: predictor_layers >= 1, predictor_kernel odd ('SAME' padding keeps the length only then)");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_fs2_pitch_destroy(maa_fs2_pitch* h) { return destroy_handle(h); }
int maa_fs2_pitch_forward(maa_ctx* ctx, maa_fs2_pitch* h, const float* d_origin, const int* d_mel2ph, const float* d_f0, const float* d_uv,
                          int B, int T_mel, float* d_decoder_inp, float* d_pitch_pred, float* d_f0_denorm, int* d_coarse) {
    return guarded([&] {
        MAA_CHECK(h && d_origin&& d_mel2ph && d_decoder_inp && d_pitch_pred && d_f0_denorm, "bad fs2_pitch_forward arguments: null pointer");
        MAA_CHECK(B > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_pitch_forward arguments: B, T_mel");
        MAA_CHECK(d_decoder_inp != d_origin, "bad fs2_pitch_forward arguments: d_decoder_inp may not alias d_origin");
        bind(ctx);
        h->m->forward(ctx->c, d_origin, d_origin, d_mel2ph, d_f0, d_uv, B, T_mel, d_decoder_inp, d_pitch_pred, d_f0_denorm, d_coarse);
    });
}
int maa_fs2_pitch_forward_from(maa_ctx* ctx, maa_fs2_pitch* h, const float* d_pred_inp, const float* d_origin, const int* d_mel2ph,
                               const float* d_f0, const float* d_uv, int B, int T_mel, float* d_decoder_inp, float* d_pitch_pred,
                               float* d_f0_denorm, int* d_coarse) {
    return guarded([&] {
        MAA_CHECK(h && d_pred_inp && d_origin && d_mel2ph && d_decoder_inp && d_pitch_pred && d_f0_denorm,
                  "bad fs2_pitch_forward_from arguments: null pointer");
        MAA_CHECK(B > 0 && T_mel > 0 && (long long)B * T_mel < (1LL << 31) / 4096, "bad fs2_pitch_forward_from arguments: B, T_mel");
        MAA_CHECK(d_decoder_inp != d_origin && d_decoder_inp != d_pred_inp,
                  "bad fs2_pitch_forward_from arguments: d_decoder_inp may not alias d_origin or d_pred_inp");
        bind(ctx);
        h->m->forward(ctx->c, d_pred_inp, d_origin, d_mel2ph, d_f0, d_uv, B, T_mel, d_decoder_inp, d_pitch_pred, d_f0_denorm, d_coarse);
    });
}

// ------------------------------------------------------------------------------------------ conditioning encoders
int maa_encoder_create(maa_ctx* ctx, const maa_encoder_config* cfg, const maa_tensor* tensors, int n_tensors,
                       maa_encoder** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out && cfg->kind >= 0 && cfg->kind <= 2 && cfg->layers > 0 && cfg->width > 0 && cfg->heads > 0 &&
                      cfg->width % cfg->heads == 0 && cfg->width % 4 == 0 && cfg->mlp_dim > 0 && cfg->d_proj > 0 &&
                      cfg->d_proj % 4 == 0 && cfg->ln_eps > 0.f,
                  "bad encoder config");
        if (cfg->kind != 1)
            MAA_CHECK(cfg->vocab > 0 && cfg->max_positions > 0, "bad text encoder config");
        else
            MAA_CHECK(cfg->patch > 0 && cfg->image > 0 && cfg->image % cfg->patch == 0, "bad image encoder config");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_encoder_destroy(maa_encoder* e) { return destroy_handle(e); }
int maa_encoder_text(maa_ctx* ctx, maa_encoder* e, const int* d_ids, int B, int L, float* d_out) {
    return guarded([&] {
        MAA_CHECK(e && d_ids && d_out && B > 0 && L > 0, "bad encoder_text arguments");
        bind(ctx);
        e->m->text(ctx->c, d_ids, B, L, d_out);
    });
}
int maa_encoder_image(maa_ctx* ctx, maa_encoder* e, const float* d_img, int B, float* d_out) {
    return guarded([&] {
        MAA_CHECK(e && d_img && d_out && B > 0, "bad encoder_image arguments");
        bind(ctx);
        e->m->image(ctx->c, d_img, B, d_out);
    });
}

int maa_encoder_text_cls(maa_ctx* ctx, maa_encoder* e, const int* d_ids, int B, int L, float* d_out) {
    return guarded([&] {
        MAA_CHECK(e && d_ids && d_out && B > 0 && L > 0, "bad encoder_text_cls arguments");
        bind(ctx);
        e->m->text_cls(ctx->c, d_ids, B, L, d_out);
    });
}

int maa_clap_audio_create(maa_ctx* ctx, const maa_clap_audio_config* cfg, const maa_tensor* tensors, int n_tensors,
                          maa_clap_audio** out) {
    return guarded([&] {
        MAA_CHECK(cfg && out && cfg->mel_bins > 0 && cfg->n_blocks > 0 && cfg->n_blocks <= 8 && cfg->out_emb > 0 &&
                      cfg->d_proj > 0 && cfg->d_proj % 4 == 0 && cfg->bn_eps > 0.f,
                  "bad clap_audio config");
        for (int i = 0; i < cfg->n_blocks; ++i) MAA_CHECK(cfg->channels[i] > 0, "bad clap_audio channel list");
        auto sd = to_state_dict(tensors, n_tensors);
        bind(ctx);
        create_handle(out, *cfg, sd, ctx->c.dtype);
    });
}
int maa_clap_audio_destroy(maa_clap_audio* a) { return destroy_handle(a); }
int maa_clap_audio_embed(maa_ctx* ctx, maa_clap_audio* a, const float* d_logmel, int B, int T, float* d_embedding,
                         float* d_z) {
    return guarded([&] {
        MAA_CHECK(a && d_logmel && d_z && B > 0 && T > 0, "bad clap_audio_embed arguments");
        bind(ctx);
        a->m->embed(ctx->c, d_logmel, B, T, d_embedding, d_z);
    });
}
int maa_clap_similarity(maa_ctx* ctx, const float* d_audio, const float* d_text, int Na, int Nt, int D, float scale,
                        float* d_out) {
    return guarded([&] {
        MAA_CHECK(d_audio && d_text && d_out && Na > 0 && Nt > 0 && D > 0, "bad clap_similarity arguments");
        bind(ctx);
        maa::launch_similarity(ctx->c, d_audio, d_text, Na, Nt, D, scale, d_out);
    });
}

int maa_spectral_create(maa_ctx* ctx, const maa_spectral_config* cfg, const float* h_basis, const float* h_melw,
                        maa_spectral** out) {
    return guarded([&] {
        MAA_CHECK(cfg && h_basis && h_melw && out, "bad spectral arguments");
        MAA_CHECK(cfg->n_fft > 0 && cfg->n_fft % 4 == 0 && cfg->hop > 0 && cfg->hop % 4 == 0 && cfg->n_freq == cfg->n_fft / 2 + 1 &&
                      cfg->n_mels > 0 && (cfg->pad_mode == 0 || cfg->pad_mode == 1) && (cfg->power == 1 || cfg->power == 2) &&
                      (cfg->log_kind == 0 || cfg->log_kind == 1) && cfg->amin > 0.f && (cfg->out_layout == 0 || cfg->out_layout == 1),
                  "bad spectral config (n_fft and hop must be multiples of 4)");
        bind(ctx);
        create_handle(out, *cfg, h_basis, h_melw);
    });
}
int maa_spectral_destroy(maa_spectral* s) { return destroy_handle(s); }
int maa_spectral_forward(maa_ctx* ctx, maa_spectral* s, const float* d_wav, int B, int n, float* d_out) {
    return guarded([&] {
        MAA_CHECK(s && d_wav && d_out && B > 0 && n > 0, "bad spectral_forward arguments");
        bind(ctx);
        MAA_CHECK(s->m->config().pad_mode == 0 || n > s->m->config().n_fft / 2, "signal too short for reflect padding");
        s->m->forward(ctx->c, d_wav, B, n, d_out);
    });
}

int maa_resampler_create(maa_ctx* ctx, int orig, int neu, int width, int klen, const float* h_kernels, maa_resampler** out) {
    return guarded([&] {
        MAA_CHECK(out && h_kernels && orig > 0 && neu > 0 && width > 0 && klen > 0, "bad resampler arguments");
        bind(ctx);
        create_handle(out, orig, neu, width, klen, h_kernels);
    });
}
int maa_resampler_destroy(maa_resampler* r) { return destroy_handle(r); }
int maa_resampler_forward(maa_ctx* ctx, maa_resampler* r, const float* d_wav, int B, int n, float* d_out) {
    return guarded([&] {
        MAA_CHECK(r && d_wav && d_out && B > 0 && n > 0, "bad resampler_forward arguments");
        bind(ctx);
        r->m->forward(ctx->c, d_wav, B, n, d_out);
    });
}

// MAA_OP_PRESPLIT=1 (tests): hand the activation to the contraction in the split32 form a normalisation would
// have written, so the op entry points exercise the LDS-DMA engines too.
static bool op_presplit(const maa::Ctx& c, int channels, bool other_prologue) {
    return c.tune.op_presplit && c.dtype != 0 && channels % 32 == 0 && !other_prologue;
}

int maa_op_linear(maa_ctx* ctx, const float* d_a, int M, int K, const float* h_w, const float* h_bias, int N,
                  int geglu, float* d_y, const float* d_res, int c_split) {
    return guarded([&] {
        MAA_CHECK(d_a && h_w && d_y && M > 0 && K > 0 && N > 0, "bad op_linear arguments");
        MAA_CHECK(!c_split || N % 32 == 0, "op_linear: split32 output needs a multiple of 32 columns");
        MAA_CHECK(!geglu || (!d_res && !c_split), "op_linear: GEGLU takes neither a residual nor split32 output here");
        MAA_CHECK(!geglu || h_bias, "geglu needs a bias");
        bind(ctx);
        OneShot s;
        s.add("w", h_w, {N, K});
        if (h_bias) s.add("b", h_bias, {N});
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        maa::PackedW pw = geglu ? ws.pack_geglu(s.sd, "w", "b") : ws.pack_conv(s.sd, "w", h_bias ? "b" : "", 1, 1);
        const bool pre = op_presplit(c, K, false);
        maa::run_sized(c, [&] {
            const float* a = d_a;
            if (pre) {
                float* sp = c.ws.alloc_f((size_t)M * K);
                maa::launch_split32_pack(c, d_a, M, K, sp);
                a = sp;
            }
            maa::LinOpt o(pre, c_split);
            o.geglu = geglu;
            maa::linear_into(c, a, K, M, K, pw, d_res, N, d_y, geglu ? N / 2 : N, o);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_conv(maa_ctx* ctx, const float* d_x, int B, int Cin, int H, int W, const float* h_w, const float* h_bias,
                int Cout, int KH, int KW, int stride, int pad, int dil, int upsample2, float leaky_slope, float* d_y,
                int Ho, int Wo, const float* d_rowadd, const float* d_res, int c_split) {
    return guarded([&] {
        MAA_CHECK(d_x && h_w && d_y, "bad op_conv arguments");
        const bool extras = d_rowadd || d_res || c_split;
        MAA_CHECK(!extras || !upsample2, "op_conv: row add, residual and split32 output are not combined with the upsample");
        MAA_CHECK(!c_split || Cout % 32 == 0, "op_conv: split32 output needs a multiple of 32 channels");
        bind(ctx);
        OneShot s;
        s.add("w", h_w, {Cout, Cin, KH, KW});
        if (h_bias) s.add("b", h_bias, {Cout});
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        maa::PackedW pw = ws.pack_conv(s.sd, "w", h_bias ? "b" : "", KH, KW);
        const bool plain3x3 = KH == 3 && KW == 3 && stride == 1 && pad == 1 && dil == 1;
        maa::PackedW pw4;      // Upsample + conv3x3: the four-phase form the models take in the bf16 modes (blocks.cpp conv_up2_into)
        if (upsample2 && plain3x3 && leaky_slope == 0.f) pw4 = ws.pack_conv_up2(s.sd, "w", h_bias ? "b" : "");
        const bool presplit = !pw4.w && op_presplit(c, Cin, leaky_slope != 0.f);
        maa::PackedW pn;       // the UNet's output convolution on its own kernel (unet.cpp finish), packed once, outside the sized run
        if (presplit && Cout <= 4 && h_bias && plain3x3 && !upsample2 && !extras && c.tune.up2) pn = ws.pack_narrow3x3(s.sd, "w", "b");
        maa::run_sized(c, [&] {
            maa::T4 x = maa::alloc_t(c, B, H, W, Cin);
            maa::launch_nchw_to_nhwc(c, d_x, B, Cin, H * W, x.p);
            if (presplit) {
                maa::T4 xs = maa::alloc_t(c, B, H, W, Cin);
                maa::launch_split32_pack(c, x.p, (long long)B * H * W, Cin, xs.p);
                xs.split = true;
                x = xs;
            }
            if (pn.w && maa::launch_narrow_conv3x3(c, x.p, Cin, B, H, W, Cin, pn.w, pn.bias, Cout, d_y)) return;
            maa::T4 y = maa::alloc_t(c, B, Ho, Wo, Cout);
            maa::ConvOpt o;
            o.KH = KH;
            o.KW = KW;
            o.stride = stride;
            o.pad = pad;
            o.dil = dil;
            o.up = upsample2;
            if (leaky_slope != 0.f) {
                o.a_act = 1;
                o.a_slope = leaky_slope;
            }
            o.rowadd = d_rowadd;      // [B, Cout]: the time-embedding row of a ResBlock's first convolution
            o.ld_rowadd = Cout;
            if (d_res) {
                maa::T4 r = maa::alloc_t(c, B, Ho, Wo, Cout);
                maa::launch_nchw_to_nhwc(c, d_res, B, Cout, Ho * Wo, r.p);
                o.res = r.p;
            }
            if (c_split) {             // the result stays channels-last: d_y = [B Ho Wo][Cout] split32 rows
                o.c_split = 1;
                y.p = d_y;
                maa::conv_into(c, x, nullptr, pw, o, y);
                return;
            }
            if (!(pw4.w && maa::conv_up2_into(c, x, pw4, y))) maa::conv_into(c, x, nullptr, pw, o, y);
            maa::launch_nhwc_to_nchw(c, y.p, B, Cout, Ho * Wo, d_y, Cout);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_igemm_ex(maa_ctx* ctx, const maa_igemm_ex_args* a) {
    return guarded([&] {
        MAA_CHECK(a && a->d_x1 && a->h_w && a->d_c, "bad op_igemm_ex arguments: null pointer");
        MAA_CHECK(a->B > 0 && a->H > 0 && a->W > 0 && a->Ho > 0 && a->Wo > 0 && a->C1 > 0 && a->C2 >= 0 && a->Cout > 0 && a->KH > 0 &&
                      a->KW > 0 && a->stride > 0 && a->dil > 0 && a->pad_w >= 0 && a->pad_h >= -1,
                  "bad op_igemm_ex sizes");
        MAA_CHECK((long long)a->B * a->Ho * a->Wo < (1ll << 31) && (long long)a->KH * a->KW * (a->C1 + a->C2) < (1ll << 31), "bad op_igemm_ex sizes");
        MAA_CHECK((a->C2 == 0) == (a->d_x2 == nullptr), "op_igemm_ex: a second source needs both d_x2 and C2");
        MAA_CHECK(!a->geglu || (a->h_bias && a->KH == 1 && a->KW == 1 && a->Cout % 2 == 0), "op_igemm_ex: GEGLU is a biased linear of 2 * inner columns");
        const int N = a->geglu ? a->Cout / 2 : a->Cout, Ctot = a->C1 + a->C2;
        MAA_CHECK(a->ld1 >= a->C1 && (a->C2 == 0 || a->ld2 >= a->C2) && a->ldc >= N && (!a->d_res || a->ldr >= N) &&
                      (!a->d_c2 || a->ldc2 >= N) && (!a->d_rowadd || a->ld_rowadd >= N),
                  "op_igemm_ex: a pitch is smaller than its width");
        MAA_CHECK(!a->presplit || (a->C2 == 0 && a->C1 % 32 == 0 && a->ld1 == a->C1),
                  "op_igemm_ex: presplit takes one dense source of whole 32-channel lines");
        bind(ctx);
        maa::Ctx& c = ctx->c;
        MAA_CHECK(!a->presplit || c.dtype != 0, "op_igemm_ex: presplit needs a bf16 mode");
        OneShot s;
        if (a->geglu)
            s.add("w", a->h_w, {a->Cout, Ctot});
        else
            s.add("w", a->h_w, {a->Cout, Ctot, a->KH, a->KW});
        if (a->h_bias) s.add("b", a->h_bias, {a->Cout});
        maa::WeightStore ws(c.dtype != 0);
        maa::PackedW pw = a->geglu ? ws.pack_geglu(s.sd, "w", "b") : ws.pack_conv(s.sd, "w", a->h_bias ? "b" : "", a->KH, a->KW);
        maa::run_sized(c, [&] {
            maa::T4 x1, x2, y;
            x1.p = const_cast<float*>(a->d_x1);
            x1.B = a->B;
            x1.H = a->H;
            x1.W = a->W;
            x1.C = a->C1;
            x1.ld = a->ld1;
            x2 = x1;
            x2.p = const_cast<float*>(a->d_x2);
            x2.C = a->C2;
            x2.ld = a->ld2;
            maa::ConvOpt o;
            if (a->a_leaky != 0.f) {
                o.a_act = 1;
                o.a_slope = a->a_leaky;
            }
            if (a->presplit) {      // the slope goes into the packed rows: the engines that take split32 A apply no activation
                float* xs = c.ws.alloc_f((size_t)a->B * a->H * a->W * a->C1);
                maa::launch_split32_pack(c, a->d_x1, (long long)a->B * a->H * a->W, a->C1, xs, a->a_leaky != 0.f ? a->a_leaky : 1.f);
                x1.p = xs;
                x1.ld = 0;
                x1.split = true;
                o.a_act = 0;
            }
            y.p = a->d_c;
            y.B = a->B;
            y.H = a->Ho;
            y.W = a->Wo;
            y.C = N;
            o.KH = a->KH;
            o.KW = a->KW;
            o.stride = a->stride;
            o.pad = a->pad_w;
            o.pad_h = a->pad_h;
            o.dil = a->dil;
            o.up = a->up ? 1 : 0;
            o.alpha = a->alpha;
            o.rowadd = a->d_rowadd;
            o.ld_rowadd = a->ld_rowadd;
            o.res = a->d_res;
            o.ldr = a->ldr;
            o.act = a->act;
            o.act_slope = a->act_slope;
            o.out_scale = a->out_scale;
            o.accumulate = a->accumulate ? 1 : 0;
            o.geglu = a->geglu ? 1 : 0;
            o.c_split = a->c_split ? 1 : 0;
            o.ldc = a->ldc;
            o.c2 = a->d_c2;
            o.ldc2 = a->ldc2;
            o.c2_slope = a->c2_slope;
            maa::conv_into(c, x1, a->d_x2 ? &x2 : nullptr, pw, o, y);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_calib(maa_ctx* ctx, int kind, double* out_value) {
    return guarded([&] {
        MAA_CHECK(out_value && kind >= 0 && kind <= 3, "bad calib arguments");
        bind(ctx);
        *out_value = maa::calib_run(ctx->c, kind);
    });
}

int maa_op_groupnorm(maa_ctx* ctx, const float* d_x, int B, int C, int HW, const float* h_gamma, const float* h_beta,
                     float eps, int silu, float* d_y) {
    return guarded([&] {
        MAA_CHECK(d_x && h_gamma && h_beta && d_y, "bad op_groupnorm arguments");
        bind(ctx);
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        float* g = ws.upload(std::vector<float>(h_gamma, h_gamma + C));
        float* b = ws.upload(std::vector<float>(h_beta, h_beta + C));
        maa::run_sized(c, [&] {
            maa::T4 x = maa::alloc_t(c, B, 1, HW, C), y = maa::alloc_t(c, B, 1, HW, C);
            maa::launch_nchw_to_nhwc(c, d_x, B, C, HW, x.p);
            maa::launch_groupnorm(c, x.p, C, C, nullptr, 0, 0, B, HW, 32, g, b, eps, silu, y.p);
            maa::launch_nhwc_to_nchw(c, y.p, B, C, HW, d_y, C);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_layernorm(maa_ctx* ctx, const float* d_x, int rows, int C, const float* h_gamma, const float* h_beta,
                     float eps, float* d_y) {
    return guarded([&] {
        MAA_CHECK(d_x && h_gamma && h_beta && d_y, "bad op_layernorm arguments");
        bind(ctx);
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        float* g = ws.upload(std::vector<float>(h_gamma, h_gamma + C));
        float* b = ws.upload(std::vector<float>(h_beta, h_beta + C));
        maa::launch_layernorm(c, d_x, rows, C, g, b, eps, d_y);
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_attention(maa_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, int B, int heads, int dh,
                     int Nq, int Nk, float alpha, float* d_y) {
    return guarded([&] {
        MAA_CHECK(d_q && d_k && d_v && d_y, "bad op_attention arguments");
        bind(ctx);
        maa::Ctx& c = ctx->c;
        const int C = heads * dh;
        maa::run_sized(c, [&] {
            maa::attention_into(c, d_q, C, dh, d_k, C, dh, d_v, C, dh, B, heads, dh, Nq, Nk, alpha, d_y, C);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_attention_ex(maa_ctx* ctx, const float* d_q, int ldq, int hsq, const float* d_k, int ldk, int hsk,
                        const float* d_v, int ldv, int hsv, int B, int heads, int dh, int Nq, int Nk, float alpha,
                        float* d_y, int ldo, int out_split, int causal) {
    return guarded([&] {
        MAA_CHECK(d_q && d_k && d_v && d_y, "bad op_attention_ex arguments");
        MAA_CHECK(B > 0 && heads > 0 && dh > 0 && Nq > 0 && Nk > 0, "bad op_attention_ex sizes");
        MAA_CHECK(ldq >= dh && ldk >= dh && ldv >= dh && hsq >= 0 && hsk >= 0 && hsv >= 0 && ldo >= heads * dh,
                  "bad op_attention_ex strides");
        bind(ctx);
        maa::Ctx& c = ctx->c;
        maa::run_sized(c, [&] {
            maa::attention_into(c, d_q, ldq, hsq, d_k, ldk, hsk, d_v, ldv, hsv, B, heads, dh, Nq, Nk, alpha, d_y, ldo,
                                out_split, causal);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_attention_masked(maa_ctx* ctx, const float* d_q, int ldq, int hsq, const float* d_k, int ldk, int hsk,
                            const float* d_v, int ldv, int hsv, int B, int heads, int dh, int Nq, int Nk, float alpha,
                            float* d_y, int ldo, int out_split, int causal, const float* d_key_mask) {
    return guarded([&] {
        MAA_CHECK(d_q && d_k && d_v && d_y && d_key_mask, "bad op_attention_masked arguments");
        MAA_CHECK(B > 0 && heads > 0 && dh > 0 && Nq > 0 && Nk > 0, "bad op_attention_masked sizes");
        MAA_CHECK(ldq >= dh && ldk >= dh && ldv >= dh && hsq >= 0 && hsk >= 0 && hsv >= 0 && ldo >= heads * dh,
                  "bad op_attention_masked strides");
        bind(ctx);
        maa::Ctx& c = ctx->c;
        maa::run_sized(c, [&] {
            maa::attention_into(c, d_q, ldq, hsq, d_k, ldk, hsk, d_v, ldv, hsv, B, heads, dh, Nq, Nk, alpha, d_y, ldo,
                                out_split, causal, d_key_mask);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_groupnorm_ex(maa_ctx* ctx, const float* d_x1, int ld1, int C1, const float* d_x2, int ld2, int C2, int B, int HW,
                        int groups, const float* h_gamma, const float* h_beta, float eps, int silu, float* d_y, int out_split,
                        float* d_raw) {
    return guarded([&] {
        MAA_CHECK(d_x1 && h_gamma && h_beta && d_y, "bad op_groupnorm_ex arguments");
        MAA_CHECK(B > 0 && HW > 0 && groups > 0 && C1 > 0 && C2 >= 0 && eps > 0.f, "bad op_groupnorm_ex sizes");
        MAA_CHECK((C2 == 0) == (d_x2 == nullptr), "op_groupnorm_ex: a second source needs both d_x2 and C2");
        MAA_CHECK(ld1 >= C1 && (C2 == 0 || ld2 >= C2), "bad op_groupnorm_ex strides");
        const int C = C1 + C2;
        MAA_CHECK(C % groups == 0 && C / groups <= 256 && C1 % 4 == 0 && C2 % 4 == 0 && ld1 % 4 == 0 && ld2 % 4 == 0,
                  "op_groupnorm_ex: channels and pitches in whole float4s, at most 256 channels per group");
        MAA_CHECK((!out_split && !d_raw) || C % 32 == 0, "op_groupnorm_ex: split32 rows are whole 32-channel lines");
        MAA_CHECK((reinterpret_cast<uintptr_t>(d_x1) | reinterpret_cast<uintptr_t>(d_x2) | reinterpret_cast<uintptr_t>(d_y) |
                   reinterpret_cast<uintptr_t>(d_raw)) % 16 == 0, "op_groupnorm_ex: buffers must be 16-byte aligned");
        bind(ctx);
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        float* g = ws.upload(std::vector<float>(h_gamma, h_gamma + C));
        float* b = ws.upload(std::vector<float>(h_beta, h_beta + C));
        maa::run_sized(c, [&] {
            maa::launch_groupnorm(c, d_x1, ld1, C1, d_x2, ld2, C2, B, HW, groups, g, b, eps, silu, d_y, out_split ? 1 : 0, d_raw);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_layernorm_ex(maa_ctx* ctx, const float* d_x, int rows, int C, const float* h_gamma, const float* h_beta, float eps,
                        float* d_y, int out_split) {
    return guarded([&] {
        MAA_CHECK(d_x && h_gamma && h_beta && d_y, "bad op_layernorm_ex arguments");
        MAA_CHECK(rows > 0 && C > 0 && C % 4 == 0 && C <= 2048 && eps > 0.f, "bad op_layernorm_ex sizes");
        MAA_CHECK(!out_split || C % 32 == 0, "op_layernorm_ex: split32 rows are whole 32-channel lines");
        bind(ctx);
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        float* g = ws.upload(std::vector<float>(h_gamma, h_gamma + C));
        float* b = ws.upload(std::vector<float>(h_beta, h_beta + C));
        maa::launch_layernorm(c, d_x, rows, C, g, b, eps, d_y, out_split ? 1 : 0);
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_seq_rows(maa_ctx* ctx, const maa_seq_rows_args* a) {
    return guarded([&] {
        MAA_CHECK(a != nullptr, "bad op_seq_rows arguments: null pointer");
        const int k = a->kind;
        MAA_CHECK(k >= MAA_SEQ_FRAME_MASK && k <= MAA_SEQ_HEAD, "op_seq_rows: unknown kind");
        const bool per_sample = k == MAA_SEQ_GN_RELU_RES || k == MAA_SEQ_POS_ADD;      // rows = B * T
        bool ptrs = a->d_x && a->d_out;
        if (k == MAA_SEQ_AFFINE_MASK) ptrs = ptrs && a->d_mask;
        if (k == MAA_SEQ_GN_RELU_RES) ptrs = ptrs && a->d_res && a->h_gamma && a->h_beta;
        if (k == MAA_SEQ_HEAD)
            ptrs = ptrs && a->d_mask && a->h_gamma && a->h_beta && a->h_w && a->h_bias && (a->n_out == 1 ? a->d_dur != nullptr : a->d_out2 != nullptr);
        MAA_CHECK(ptrs, "bad op_seq_rows arguments: null pointer");
        if (per_sample)
            MAA_CHECK(a->B >= 1 && a->T >= 1 && (long long)a->B * a->T < (1ll << 31), "op_seq_rows: rows < 1 (B and T must be at least 1)");
        else
            MAA_CHECK(a->rows >= 1, "op_seq_rows: rows < 1");
        MAA_CHECK(a->C >= 4 && a->C % 4 == 0, "op_seq_rows: C % 4 != 0 (channel counts are positive multiples of 4)");
        if (k == MAA_SEQ_AFFINE_MASK)
            MAA_CHECK((a->h_scale == nullptr) == (a->h_shift == nullptr), "op_seq_rows: scale and shift come both or neither");
        if (k == MAA_SEQ_GN_RELU_RES)
            MAA_CHECK(a->groups > 0 && a->C % a->groups == 0 && (a->C / a->groups) % 4 == 0 && a->C / a->groups <= 256 && a->eps > 0.f,
                      "op_seq_rows: groups must divide C into whole float4s, at most 256 channels per group");
        if (k == MAA_SEQ_POS_ADD) MAA_CHECK(a->table_rows >= 2, "op_seq_rows: table_rows < 2");
        if (k == MAA_SEQ_HEAD) {
            MAA_CHECK(a->C <= 1024, "op_seq_rows: head C > 1024");
            MAA_CHECK((a->n_out == 1 || a->n_out == 2) && a->eps > 0.f && (a->pitch_norm == 0 || a->pitch_norm == 1),
                      "op_seq_rows: the head has n_out 1 or 2, pitch_norm 0 or 1");
        }
        bind(ctx);
        maa::Ctx& c = ctx->c;
        maa::WeightStore ws(c.dtype != 0);
        const int C = a->C;
        auto up = [&](const float* h, size_t n) { return h ? ws.upload(std::vector<float>(h, h + n)) : nullptr; };
        switch (k) {
        case MAA_SEQ_FRAME_MASK:
            maa::launch_pe_frame_mask(c, a->d_x, a->rows, C, a->d_out, a->d_out2);
            break;
        case MAA_SEQ_AFFINE_MASK:
            maa::launch_pe_affine_mask(c, a->d_x, a->rows, C, up(a->h_scale, C), up(a->h_shift, C), a->d_mask, a->d_out);
            break;
        case MAA_SEQ_GN_RELU_RES: {
            const float *g = up(a->h_gamma, C), *b = up(a->h_beta, C);
            maa::run_sized(c, [&] { maa::launch_pe_gn_relu_res(c, a->d_x, a->d_res, a->B, a->T, C, a->groups, g, b, a->eps, a->d_out); });
            break;
        }
        case MAA_SEQ_POS_ADD: {
            maa::SinusoidTable table;
            table.build(ws, a->table_rows, C);
            table.grow(c, a->T);
            maa::run_sized(c, [&] { maa::launch_pe_pos_add(c, a->d_x, a->B, a->T, C, table.ptr(), a->alpha, a->d_out, a->d_pos); });
            MAA_HIP(hipStreamSynchronize(c.stream));      // (the grown table is freed with `table`)
            break;
        }
        default: {
            const float *g = up(a->h_gamma, C), *b = up(a->h_beta, C), *w = up(a->h_w, (size_t)a->n_out * C), *bi = up(a->h_bias, a->n_out);
            if (a->n_out == 2)
                maa::launch_pe_head(c, a->d_x, a->rows, C, g, b, a->eps, w, bi, a->d_mask, a->pitch_norm, a->f0_mean, a->f0_std, a->use_uv,
                                    a->d_out, a->d_out2);
            else
                maa::launch_fs2_dur_head(c, a->d_x, a->rows, C, g, b, a->eps, w, bi, a->d_mask, a->d_out, a->d_dur);
        }
        }
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_tts_rows(maa_ctx* ctx, const maa_tts_rows_args* a) {
    return guarded([&] {
        MAA_CHECK(a != nullptr, "bad op_tts_rows arguments: null pointer");
        const int k = a->kind;
        MAA_CHECK(k >= MAA_TTS_GLOW_SQUEEZE && k <= MAA_TTS_FS2_TGT_MASK, "op_tts_rows: unknown kind");
        const bool per_sample = k == MAA_TTS_GLOW_SQUEEZE || k == MAA_TTS_GLOW_LOGDET || k == MAA_TTS_FS2_EMBED_PLAIN ||
                                k == MAA_TTS_FS2_ADD_SPEAKER;                                      // rows = B * T
        const bool head = k == MAA_TTS_FS2_ENERGY_TAIL && a->d_x != nullptr;
        bool ptrs = a->d_out != nullptr;
        if (k <= MAA_TTS_GLOW_LOGDET || k == MAA_TTS_FS2_ADD_SPEAKER) ptrs = ptrs && a->d_x;
        if (k == MAA_TTS_GLOW_WN_RESIDUAL) ptrs = ptrs && a->d_mask && a->d_out2;
        if (k == MAA_TTS_GLOW_BLOCK_TAIL) ptrs = ptrs && a->d_y && a->d_mask && a->h_winv && a->h_an_bias && a->h_an_einv && a->d_rowld;
        if (k == MAA_TTS_GLOW_LOGDET) ptrs = ptrs && a->d_mask;
        if (k == MAA_TTS_FS2_EMBED_PLAIN) ptrs = ptrs && a->d_tok && a->h_table && a->h_pe && a->d_out2 && a->d_out3;
        if (k == MAA_TTS_FS2_ADD_SPEAKER) ptrs = ptrs && a->d_spk && (a->d_mask || a->d_mel2ph);
        if (k == MAA_TTS_FS2_SPEAKER_GATHER) ptrs = ptrs && a->h_table && a->h_t1 && a->h_t2;
        if (k == MAA_TTS_FS2_ENERGY_TAIL) ptrs = ptrs && a->d_y && a->d_mel2ph;
        if (head) ptrs = ptrs && a->h_gamma && a->h_beta && a->h_w && a->h_bias && a->h_table;
        if (k == MAA_TTS_FS2_TGT_MASK) ptrs = ptrs && a->d_mel2ph;
        MAA_CHECK(ptrs, "bad op_tts_rows arguments: null pointer");
        if (per_sample)
            MAA_CHECK(a->B >= 1 && a->T >= 1 && (long long)a->B * a->T < (1ll << 31), "op_tts_rows: rows < 1 (B and T must be at least 1)");
        else if (k == MAA_TTS_FS2_SPEAKER_GATHER)
            MAA_CHECK(a->B >= 1, "op_tts_rows: rows < 1 (B must be at least 1)");
        else
            MAA_CHECK(a->rows >= 1, "op_tts_rows: rows < 1");
        if (k == MAA_TTS_GLOW_SQUEEZE) MAA_CHECK(a->T >= 2, "op_tts_rows: T < 2 (the squeeze pairs frames)");
        if (k != MAA_TTS_GLOW_LOGDET && k != MAA_TTS_FS2_TGT_MASK && (k != MAA_TTS_FS2_ENERGY_TAIL || head))
            MAA_CHECK(a->C >= 4 && a->C % 4 == 0, "op_tts_rows: C % 4 != 0 (channel counts are positive multiples of 4)");
        if (k == MAA_TTS_GLOW_WN_RESIDUAL)
            MAA_CHECK((a->first == 0 || a->first == 1) && (a->last == 0 || a->last == 1), "op_tts_rows: first and last are 0 or 1");
        if (k == MAA_TTS_GLOW_BLOCK_TAIL)
            MAA_CHECK((a->first == 0 || a->first == 1) && (a->sigmoid_scale == 0 || a->sigmoid_scale == 1),
                      "op_tts_rows: first and sigmoid_scale are 0 or 1");
        if (k == MAA_TTS_FS2_EMBED_PLAIN) {
            MAA_CHECK(a->rel == 0 || a->rel == 1, "op_tts_rows: rel is 0 or 1");
            MAA_CHECK(a->vocab >= 1, "op_tts_rows: vocab < 1");
            MAA_CHECK(a->pe_rows >= a->T + (a->rel ? 0 : 1), "op_tts_rows: pe_rows too small (T rows with rel, T + 1 without)");
        }
        if (k == MAA_TTS_FS2_ADD_SPEAKER)
            MAA_CHECK((a->d_mask == nullptr) != (a->d_mel2ph == nullptr), "op_tts_rows: mask or mel2ph, not both");
        if (k == MAA_TTS_FS2_SPEAKER_GATHER) {
            MAA_CHECK(a->split == 0 || a->split == 1, "op_tts_rows: split is 0 or 1");
            MAA_CHECK(a->n_rows >= 1 && (a->d_ids || a->n_rows >= a->B), "op_tts_rows: n_rows < 1, or < B without ids");
        }
        if (k == MAA_TTS_FS2_ENERGY_TAIL) {
            MAA_CHECK(a->H >= 4 && a->H % 4 == 0, "op_tts_rows: H % 4 != 0 (channel counts are positive multiples of 4)");
            MAA_CHECK(a->T >= 1 && a->rows % a->T == 0, "op_tts_rows: rows % T != 0 (rows is whole samples of T >= 1 frames)");
            if (head) MAA_CHECK(a->C <= 1024 && a->eps > 0.f, "op_tts_rows: energy head C > 1024 or eps <= 0");
        }
        bind(ctx);
        maa::Ctx& c = ctx->c;
        maa::WeightStore ws(c.dtype != 0);
        const int C = a->C;
        auto up = [&](const float* h, size_t n) { return h ? ws.upload(std::vector<float>(h, h + n)) : nullptr; };
        switch (k) {
        case MAA_TTS_GLOW_SQUEEZE:
            maa::launch_glow_squeeze(c, a->d_x, a->d_mask, a->B, a->T, C, a->d_out, a->d_out2);
            break;
        case MAA_TTS_GLOW_GATE:
            maa::launch_glow_gate(c, a->d_x, a->rows, C, a->d_out);
            break;
        case MAA_TTS_GLOW_WN_RESIDUAL:
            maa::launch_glow_wn_residual(c, a->d_x, a->rows, C, a->d_mask, a->first != 0, a->last != 0, a->d_out, a->d_out2);
            break;
        case MAA_TTS_GLOW_BLOCK_TAIL:
            maa::launch_glow_block_tail(c, a->d_x, a->d_y, a->d_mask, a->rows, C, a->sigmoid_scale, up(a->h_winv, 16),
                                        up(a->h_an_bias, 2 * (size_t)C), up(a->h_an_einv, 2 * (size_t)C), a->first != 0, a->d_out,
                                        a->d_rowld, a->d_h_cpl, a->d_h_inv, a->d_h_act);
            break;
        case MAA_TTS_GLOW_LOGDET:
            maa::launch_glow_logdet(c, a->d_x, a->d_mask, a->B, a->T, a->alpha, a->d_out);
            break;
        case MAA_TTS_FS2_EMBED_PLAIN: {
            const float *E = up(a->h_table, (size_t)a->vocab * C), *pe = up(a->h_pe, (size_t)a->pe_rows * C);
            maa::run_sized(c, [&] {
                maa::launch_fs2_embed_plain(c, a->d_tok, E, a->vocab, pe, a->alpha, a->rel, a->B, a->T, C, a->d_out, a->d_out2, a->d_out3);
            });
            break;
        }
        case MAA_TTS_FS2_ADD_SPEAKER:
            maa::launch_fs2_add_speaker(c, a->d_x, a->d_spk, a->d_mel2ph, a->d_mask, a->B, a->T, C, a->d_out);
            break;
        case MAA_TTS_FS2_SPEAKER_GATHER: {
            const size_t n = (size_t)a->n_rows * C;
            maa::launch_fs2_speaker_gather(c, up(a->h_table, n), up(a->h_t1, n), up(a->h_t2, n), a->d_ids, a->split, a->n_rows, a->B, C,
                                           a->d_out);
            break;
        }
        case MAA_TTS_FS2_ENERGY_TAIL: {
            const float *g = nullptr, *b = nullptr, *w = nullptr, *bi = nullptr, *tab = nullptr;
            if (head) g = up(a->h_gamma, C), b = up(a->h_beta, C), w = up(a->h_w, C), bi = up(a->h_bias, 1), tab = up(a->h_table, 256 * (size_t)a->H);
            maa::launch_fs2_energy_tail(c, a->d_x, a->rows, C, g, b, a->eps, w, bi, a->d_mel2ph, a->d_energy, a->d_y, tab, a->d_spk, a->T,
                                        a->H, a->d_energy_pred, a->d_bin, a->d_out);
            break;
        }
        default:
            maa::launch_fs2_tgt_mask(c, a->d_mel2ph, a->rows, a->d_out);
        }
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_sampler_step(maa_ctx* ctx, const maa_sampler_step_args* a) {
    return guarded([&] {
        MAA_CHECK(a != nullptr, "bad op_sampler_step arguments: null pointer");
        const int k = a->kind;
        MAA_CHECK(k >= MAA_STEP_DDIM_PREPARE && k <= MAA_STEP_DS_DDPM, "op_sampler_step: unknown kind");
        const bool ds = k >= MAA_STEP_DS_PLMS;
        const bool rows = k == MAA_STEP_DDIM_PREPARE || k == MAA_STEP_DDIM || k == MAA_STEP_PLMS || k == MAA_STEP_PLMS_EULER_MID ||
                          k == MAA_STEP_DDPM;                                   // reads or writes d_xin [nB, per_in]
        const bool stepped = !ds && k != MAA_STEP_DDIM_PREPARE;                 // reads the coefficient slot
        bool ptrs = true;
        if (rows) ptrs = ptrs && a->d_xin;
        if (stepped) ptrs = ptrs && a->d_eps_u && a->d_coef && a->d_x;
        if (stepped && k != MAA_STEP_PLMS_EULER_MID) ptrs = ptrs && a->d_step;
        if (k == MAA_STEP_DDIM_PREPARE)
            ptrs = ptrs && a->d_x && a->d_tab_t && a->d_tab && a->d_step && a->d_cur_t && a->d_coef &&
                   (!a->d_emb_tab || a->d_cur_emb);
        if (k == MAA_STEP_PLMS) ptrs = ptrs && a->d_ring;
        if (k == MAA_STEP_PLMS_EULER_MID) ptrs = ptrs && a->d_e_keep && a->d_tab_t && a->d_cur_t && (!a->d_emb_tab || a->d_cur_emb);
        if (k == MAA_STEP_PLMS_EULER_FINAL) ptrs = ptrs && a->d_e_keep;
        if (k == MAA_STEP_DDPM) ptrs = ptrs && a->d_tab && a->d_noise_p;
        if (k == MAA_STEP_DS_PLMS) ptrs = ptrs && a->d_x && a->d_eps_u && a->d_ring && a->d_tab && a->d_st;
        if (k == MAA_STEP_DS_ADVANCE) ptrs = ptrs && a->d_st && a->d_cur_t;
        if (k == MAA_STEP_DS_DDPM) ptrs = ptrs && a->d_x && a->d_eps_u && a->d_noise_p && a->d_tab && a->d_st;
        MAA_CHECK(ptrs, "bad op_sampler_step arguments: null pointer");
        if (k != MAA_STEP_PLMS_EULER_FINAL && k != MAA_STEP_DS_PLMS && k != MAA_STEP_DS_DDPM)
            MAA_CHECK(a->B >= 1, "op_sampler_step: B < 1");
        if (rows) {
            MAA_CHECK(a->per >= 1 && a->per_in >= a->per, "op_sampler_step: per < 1 (one sample is per >= 1 floats, per_in >= per apart)");
            MAA_CHECK(a->n == (int64_t)a->B * a->per, "op_sampler_step: n % per != 0 (n is B samples of per floats)");
        } else if (k != MAA_STEP_DS_ADVANCE) {
            MAA_CHECK(a->n >= 1, "op_sampler_step: n < 1");
        }
        if (k == MAA_STEP_DDIM_PREPARE)
            MAA_CHECK(a->per_in == a->per || a->d_concat, "bad op_sampler_step arguments: null pointer (concat channels need d_concat)");
        if (k == MAA_STEP_DDIM_PREPARE || k == MAA_STEP_PLMS_EULER_MID) {
            MAA_CHECK(a->nB == a->B || a->nB == 2 * a->B, "op_sampler_step: nB is B or 2 B");
            MAA_CHECK(a->nB <= 256, "op_sampler_step: nB > 256");
            MAA_CHECK(a->emb_w >= 0 && a->n_t >= 0, "op_sampler_step: emb_w or n_t negative");
        }
        if (k == MAA_STEP_DDIM_PREPARE || k == MAA_STEP_DDIM || k == MAA_STEP_PLMS) MAA_CHECK(a->S >= 1, "op_sampler_step: S < 1");
        if (k == MAA_STEP_DDIM_PREPARE || k == MAA_STEP_DDPM)
            MAA_CHECK(!a->d_mask || (a->d_x0 && a->d_noise_q), "op_sampler_step: mask given without x0 and its noise");
        if (stepped && k != MAA_STEP_PLMS_EULER_MID)
            MAA_CHECK((a->d_log_x == nullptr) == (a->d_log_x0 == nullptr), "op_sampler_step: the two logs come both or neither");
        if (k == MAA_STEP_DS_PLMS) {
            MAA_CHECK(a->mode >= 0 && a->mode <= 2, "op_sampler_step: mode outside 0..2");
            MAA_CHECK(a->mode != 2 || a->d_e_prev, "op_sampler_step: mode 2 needs e_prev");
            MAA_CHECK(a->mode != 1 || a->d_x_out, "op_sampler_step: mode 1 needs x_out");
        }
        if (k == MAA_STEP_DS_PLMS || k == MAA_STEP_DS_ADVANCE) MAA_CHECK(a->interval >= 1, "op_sampler_step: interval < 1");
        if (k == MAA_STEP_DS_ADVANCE) MAA_CHECK(a->B <= 256, "op_sampler_step: B > 256 (the step-advance kernel is one workgroup)");
        if (k == MAA_STEP_DS_DDPM) {
            MAA_CHECK(a->timesteps >= 1 && a->n_steps >= 1, "op_sampler_step: timesteps or n_steps < 1");
            MAA_CHECK(a->n % 4 == 0 && (reinterpret_cast<uintptr_t>(a->d_x) | reinterpret_cast<uintptr_t>(a->d_eps_u) |
                                        reinterpret_cast<uintptr_t>(a->d_noise_p)) % 16 == 0,
                      "op_sampler_step: the ds ancestral step takes whole aligned float4s");
        }
        bind(ctx);
        maa::Ctx& c = ctx->c;
        switch (k) {
        case MAA_STEP_DDIM_PREPARE:
            maa::launch_ddim_prepare(c, a->d_x, a->d_concat, a->B, a->nB, a->per, a->per_in - a->per, a->d_tab_t, a->d_tab, a->d_step,
                                     a->d_xin, a->d_cur_t, a->d_coef, a->d_mask, a->d_x0, a->d_noise_q, a->S, a->d_emb_tab, a->emb_w,
                                     a->d_cur_emb, a->n_t);
            break;
        case MAA_STEP_DDIM:
            maa::launch_ddim_step(c, a->d_xin, a->per, a->per_in, a->d_eps_u, a->d_eps_c, a->scale, a->d_coef, a->n, a->d_x, a->d_noise_p,
                                  a->temperature, a->S, a->d_log_x, a->d_log_x0, a->d_step);
            break;
        case MAA_STEP_PLMS:
            maa::launch_ldm_plms_step(c, a->d_xin, a->per, a->per_in, a->d_eps_u, a->d_eps_c, a->scale, a->d_coef, a->n, a->d_x, a->d_ring,
                                      a->S, a->d_log_x, a->d_log_x0, a->d_step);
            break;
        case MAA_STEP_PLMS_EULER_MID:
            maa::launch_ldm_plms_euler_mid(c, a->d_xin, a->per, a->per_in, a->B, a->nB, a->d_eps_u, a->d_eps_c, a->scale, a->d_coef, a->d_x,
                                           a->d_e_keep, a->d_tab_t, a->d_cur_t, a->d_emb_tab, a->emb_w, a->d_cur_emb, a->n_t);
            break;
        case MAA_STEP_PLMS_EULER_FINAL:
            maa::launch_ldm_plms_euler_final(c, a->d_eps_u, a->d_eps_c, a->scale, a->d_coef, a->n, a->d_x, a->d_e_keep, a->d_log_x,
                                             a->d_log_x0, a->d_step);
            break;
        case MAA_STEP_DDPM:
            maa::launch_ddpm_step(c, a->d_xin, a->per, a->per_in, a->d_eps_u, a->d_eps_c, a->scale, a->d_coef, a->d_tab, a->n, a->d_x,
                                  a->d_noise_p, a->start, a->clip != 0, a->d_mask, a->d_x0, a->d_noise_q, a->d_log_x, a->d_log_x0,
                                  a->d_step);
            break;
        case MAA_STEP_DS_PLMS:
            maa::launch_ds_plms(c, a->d_x, a->d_eps_u, a->d_e_prev, a->d_ring, a->n, a->d_tab, a->interval, a->d_st, a->mode, a->d_x_out);
            break;
        case MAA_STEP_DS_ADVANCE:
            maa::launch_ds_plms_advance(c, a->d_st, a->interval, a->d_cur_t, a->B);
            break;
        default:
            maa::launch_ds_ddpm_step(c, a->d_x, a->d_eps_u, a->d_noise_p, a->n, a->d_tab, a->timesteps, a->d_st, a->start, a->n_steps,
                                     a->clip != 0 ? 1 : 0);
        }
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_front_rows(maa_ctx* ctx, const maa_front_rows_args* a) {
    return guarded([&] {
        MAA_CHECK(a != nullptr, "bad op_front_rows arguments: null pointer");
        const int k = a->kind;
        MAA_CHECK(k >= MAA_FRONT_PAD && k <= MAA_FRONT_POOL, "op_front_rows: unknown kind");
        MAA_CHECK(a->d_x && a->d_out && (k != MAA_FRONT_AFFINE || (a->h_scale && a->h_shift)),
                  "bad op_front_rows arguments: null pointer");
        if (k == MAA_FRONT_PAD || k == MAA_FRONT_LOGMEL || k == MAA_FRONT_POOL) MAA_CHECK(a->B >= 1, "op_front_rows: B < 1");
        if (k == MAA_FRONT_POWER) MAA_CHECK(a->rows >= 1, "op_front_rows: rows < 1");
        if (k == MAA_FRONT_PAD || k == MAA_FRONT_AFFINE) MAA_CHECK(a->n >= 1, "op_front_rows: n < 1");
        if (k == MAA_FRONT_POOL) MAA_CHECK(a->T >= 1, "op_front_rows: T < 1");
        if (k == MAA_FRONT_AFFINE || k == MAA_FRONT_POOL) MAA_CHECK(a->F >= 1, "op_front_rows: F < 1");
        if (k == MAA_FRONT_POOL) MAA_CHECK(a->C >= 1, "op_front_rows: C < 1");
        if (k == MAA_FRONT_PAD) {
            MAA_CHECK(a->mode == 0 || a->mode == 1, "op_front_rows: unknown mode");
            MAA_CHECK(a->left >= 0, "op_front_rows: left < 0");
            MAA_CHECK((long long)a->total >= (long long)a->left + a->n, "op_front_rows: total < left + n");
            MAA_CHECK(a->ldo >= a->total, "op_front_rows: ldo < total");
            // (launch_pad1d's own rule, here so that it too comes back before the context is bound)
            MAA_CHECK(a->mode == 0 || (a->n > a->left && a->n > a->total - a->left - a->n),
                      "reflect padding needs a signal longer than the pad");
        }
        if (k == MAA_FRONT_POWER) {
            MAA_CHECK(a->nf >= 1, "op_front_rows: nf < 1");
            MAA_CHECK((long long)a->ldy >= 2ll * a->nf, "op_front_rows: ldy < 2 nf");
            MAA_CHECK(a->ldm >= a->nf, "op_front_rows: ldm < nf");
        }
        if (k == MAA_FRONT_LOGMEL) {
            MAA_CHECK(a->frames >= 1, "op_front_rows: frames < 1");
            MAA_CHECK(a->n_mels >= 1, "op_front_rows: n_mels < 1");
            MAA_CHECK(a->ldmel >= a->n_mels, "op_front_rows: ldmel < n_mels");
            MAA_CHECK(a->log_kind == 0 || a->log_kind == 1, "op_front_rows: unknown log_kind");
            MAA_CHECK(a->layout == 0 || a->layout == 1, "op_front_rows: unknown layout");
            MAA_CHECK(a->amin > 0.f, "op_front_rows: amin <= 0");
        }
        bind(ctx);
        maa::Ctx& c = ctx->c;
        maa::WeightStore ws(c.dtype != 0);
        switch (k) {
        case MAA_FRONT_PAD:
            maa::launch_pad1d(c, a->d_x, a->B, a->n, a->left, a->total, a->ldo, a->mode, a->d_out);
            break;
        case MAA_FRONT_POWER:
            maa::launch_spec_power(c, a->d_x, a->rows, a->nf, a->ldy, a->ldm, a->power2, a->d_out);
            break;
        case MAA_FRONT_LOGMEL:
            maa::launch_logmel(c, a->d_x, a->B, a->frames, a->n_mels, a->ldmel, a->log_kind, a->amin, a->ref_db, a->layout, a->d_out);
            break;
        case MAA_FRONT_AFFINE: {
            const float* sc = ws.upload(std::vector<float>(a->h_scale, a->h_scale + a->F));
            const float* sh = ws.upload(std::vector<float>(a->h_shift, a->h_shift + a->F));
            maa::launch_affine_lastdim(c, a->d_x, a->n, a->F, sc, sh, a->d_out);
            break;
        }
        default:
            maa::launch_cnn14_pool(c, a->d_x, a->B, a->T, a->F, a->C, a->d_out);
        }
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_split32(maa_ctx* ctx, const float* d_x, int rows, int C, float slope, int unpack, float* d_y) {
    return guarded([&] {
        MAA_CHECK(d_x && d_y && d_x != d_y, "bad op_split32 arguments");
        MAA_CHECK(rows > 0 && C > 0 && C % 32 == 0, "op_split32: split32 rows are whole 32-channel lines");
        bind(ctx);
        maa::Ctx& c = ctx->c;
        if (unpack)
            maa::launch_split32_unpack(c, d_x, rows, C, d_y);
        else
            maa::launch_split32_pack(c, d_x, rows, C, d_y, slope);
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_unfold(maa_ctx* ctx, const float* d_x, int B, int C, int H, int W, int kh, int kw, int sh, int sw, float* d_out) {
    return guarded([&] {
        MAA_CHECK(d_x && d_out && d_x != d_out, "bad op_unfold arguments: null pointer");
        MAA_CHECK(B > 0 && C > 0, "bad op_unfold arguments: empty batch");
        maa::split_check(H, W, kh, kw, sh, sw);
        bind(ctx);
        maa::launch_split_unfold(ctx->c, d_x, B, C, H, W, kh, kw, sh, sw, d_out);
        MAA_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}

int maa_op_fold(maa_ctx* ctx, const float* d_crops, const float* h_weight, int B, int C, int H, int W, int kh, int kw, int sh, int sw,
                float* d_out) {
    return guarded([&] {
        MAA_CHECK(d_crops && h_weight && d_out && d_crops != d_out, "bad op_fold arguments: null pointer");
        MAA_CHECK(B > 0 && C > 0, "bad op_fold arguments: empty batch");
        maa::split_check(H, W, kh, kw, sh, sw);
        bind(ctx);
        maa::Ctx& c = ctx->c;
        const int L = maa::split_crops(H, W, kh, kw, sh, sw);
        const size_t kk = (size_t)kh * kw, n_w = (kk * L + 63) / 64 * 64;
        float* slab = static_cast<float*>(c.split_scratch.get((n_w + (size_t)H * W) * sizeof(float), c.stream));
        const std::vector<float> h_wT = maa::split_weight_transposed(h_weight, kk, L);
        MAA_HIP(hipMemcpyAsync(slab, h_wT.data(), h_wT.size() * sizeof(float), hipMemcpyHostToDevice, c.stream));
        maa::launch_split_norm(c, slab, H, W, kh, kw, sh, sw, slab + n_w);
        maa::launch_split_fold(c, d_crops, slab, slab + n_w, B, C, H, W, kh, kw, sh, sw, d_out);
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_conv_transpose1d(maa_ctx* ctx, const float* d_x, int B, int Cin, int L, const float* h_w,
                            const float* h_bias, int Cout, int k, int stride, float leaky_slope, float* d_y) {
    return guarded([&] {
        MAA_CHECK(d_x && h_w && h_bias && d_y && B > 0 && Cin > 0 && Cout > 0 && L > 0, "bad op_conv_transpose1d arguments");
        maa::check_convtr_polyphase(k, stride);
        bind(ctx);
        OneShot s;
        s.add("w", h_w, {Cin, Cout, k});
        s.add("b", h_bias, {Cout});
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        const int pad = (k - stride) / 2, U = k / stride;
        maa::run_sized(c, [&] {
            maa::T4 x = maa::alloc_t(c, B, 1, L, Cin), y = maa::alloc_t(c, B, 1, L * stride, Cout);
            maa::launch_nchw_to_nhwc(c, d_x, B, Cin, L, x.p);
            for (int carry = 0; carry < 2; ++carry) {
                bool any = false;
                for (int r = 0; r < stride; ++r) any = any || ((r + pad) / stride == carry);
                if (!any) continue;
                int r_start = 0, r_count = 0;
                maa::PackedW pw;
                if (!c.ws.dry) pw = ws.pack_convtr_phase(s.sd, "w", "b", stride, pad, carry, &r_start, &r_count);
                maa::IGemm p;
                p.a1 = x.p;
                p.lda1 = Cin;
                p.C1 = Cin;
                p.Win = L;
                p.Wout = L;
                p.KW = U;
                p.pw = U - 1 - carry;
                if (leaky_slope != 0.f) {
                    p.a_act = 1;
                    p.a_slope = leaky_slope;
                }
                p.b = pw.w;
                p.ldb = pw.ld;
                p.b_nk = pw.nk;
                p.b_split = pw.split;
                p.M = B * L;
                p.K = U * Cin;
                p.N = r_count * Cout;
                p.bias = pw.bias;
                p.c = y.p + (long long)r_start * Cout;
                p.ldc = stride * Cout;
                if (!c.ws.dry) maa::launch_igemm(c, p);
            }
            maa::launch_nhwc_to_nchw(c, y.p, B, Cout, L * stride, d_y, Cout);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_bench_conv(maa_ctx* ctx, int B, int H, int W, int Cin, int Cout, int taps, int pre_split, int iters,
                      float* ms_per_launch) {
    return guarded([&] {
        MAA_CHECK(ms_per_launch && iters > 0 && (taps == 1 || taps == 9), "bad op_bench_conv arguments");
        bind(ctx);
        maa::Ctx& c = ctx->c;
        const int k = taps == 9 ? 3 : 1;
        std::vector<float> hw((size_t)Cout * Cin * taps), hb(Cout, 0.1f);
        unsigned s = 12345u;
        for (auto& v : hw) {
            s = s * 1664525u + 1013904223u;
            v = ((int)(s >> 9) % 2001 - 1000) * 1e-4f;
        }
        OneShot sd;
        sd.add("w", hw.data(), {Cout, Cin, k, k});
        sd.add("b", hb.data(), {Cout});
        maa::WeightStore ws(c.dtype != 0);
        maa::PackedW pw = ws.pack_conv(sd.sd, "w", "b", k, k);
        const size_t n_in = (size_t)B * H * W * Cin, n_out = (size_t)B * H * W * Cout;
        std::vector<float> hx(n_in);
        for (auto& v : hx) {
            s = s * 1664525u + 1013904223u;
            v = ((int)(s >> 9) % 2001 - 1000) * 1e-3f;
        }
        if (pre_split && c.dtype != 0) {
            // rewrite the rows as split32 lines ([32 bf16 hi | 32 bf16 lo] per 32 channels), the GroupNorm output form
            MAA_CHECK(Cin % 32 == 0, "op_bench_conv: pre-split input needs Cin % 32 == 0");
            auto f2bf = [](float f) {
                unsigned u;
                std::memcpy(&u, &f, 4);
                u += 0x7fffu + ((u >> 16) & 1u);
                return (unsigned short)(u >> 16);
            };
            std::vector<float> packed(n_in);
            unsigned short* d = reinterpret_cast<unsigned short*>(packed.data());
            for (size_t g = 0; g < n_in / 32; ++g)
                for (int j = 0; j < 32; ++j) {
                    const float v = hx[g * 32 + j];
                    const unsigned short h = f2bf(v);
                    const unsigned hu = (unsigned)h << 16;
                    float hf;
                    std::memcpy(&hf, &hu, 4);
                    d[g * 64 + j] = h;
                    d[g * 64 + 32 + j] = f2bf(v - hf);
                }
            hx.swap(packed);
        }
        float* dx = ws.upload(hx);
        float* dy = ws.upload(std::vector<float>(n_out, 0.f));
        maa::T4 x, y;
        x.B = y.B = B;
        x.H = y.H = H;
        x.W = y.W = W;
        x.C = Cin;
        y.C = Cout;
        x.p = dx;
        y.p = dy;
        if (pre_split && c.dtype != 0) {
            x.split = true;
        }
        maa::ConvOpt o;
        o.KH = o.KW = k;
        o.pad = k / 2;
        // (the split-K engine borrows its slabs from the arena: size it with the warm-up launches)
        maa::run_sized(c, [&] {
            for (int i = 0; i < 3; ++i) maa::conv_into(c, x, nullptr, pw, o, y);
        });
        hipEvent_t e0, e1;
        MAA_HIP(hipEventCreate(&e0));
        MAA_HIP(hipEventCreate(&e1));
        MAA_HIP(hipEventRecord(e0, c.stream));
        for (int i = 0; i < iters; ++i) maa::conv_into(c, x, nullptr, pw, o, y);
        MAA_HIP(hipEventRecord(e1, c.stream));
        MAA_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        MAA_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *ms_per_launch = ms / iters;
    });
}

int maa_op_snake_aa(maa_ctx* ctx, const float* d_x, int B, int C, int L, const float* h_alpha, const float* h_beta,
                    int logscale, float* d_y) {
    return guarded([&] {
        MAA_CHECK(d_x && h_alpha && h_beta && d_y, "bad op_snake_aa arguments");
        bind(ctx);
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        std::vector<float> ha(C), hib(C);
        for (int i = 0; i < C; ++i) {
            float a = h_alpha[i], b = h_beta[i];
            if (logscale) {
                a = std::exp(a);
                b = std::exp(b);
            }
            ha[i] = a;
            hib[i] = 1.0f / (b + 1e-9f);
        }
        float* da = ws.upload(ha);
        float* dib = ws.upload(hib);
        maa::run_sized(c, [&] {
            maa::T4 x = maa::alloc_t(c, B, 1, L, C), y = maa::alloc_t(c, B, 1, L, C);
            maa::launch_nchw_to_nhwc(c, d_x, B, C, L, x.p);
            maa::launch_snake_aa(c, x.p, B, L, C, dib, da, y.p);
            maa::launch_nhwc_to_nchw(c, y.p, B, C, L, d_y, C);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

int maa_op_mrf_pair(maa_ctx* ctx, const float* d_x, int B, int C, int L, const float* h_w1, const float* h_b1, int k1, int d1,
                    float slope1, const float* h_w2, const float* h_b2, int k2, int d2, float slope2, float out_scale,
                    int accumulate, float* d_out) {
    return guarded([&] {
        MAA_CHECK(d_x && h_w1 && d_out && B > 0 && C > 0 && L > 0, "bad op_mrf_pair arguments");
        MAA_CHECK(k1 >= 1 && (k1 & 1) && d1 >= 1, "op_mrf_pair: k1 must be odd and d1 >= 1 (\"same\" padding)");
        MAA_CHECK(!h_w2 || (k2 >= 1 && (k2 & 1) && d2 >= 1), "op_mrf_pair: k2 must be odd and d2 >= 1 (\"same\" padding)");
        bind(ctx);
        OneShot s;
        s.add("w1", h_w1, {C, C, 1, k1});
        if (h_b1) s.add("b1", h_b1, {C});
        if (h_w2) s.add("w2", h_w2, {C, C, 1, k2});
        if (h_w2 && h_b2) s.add("b2", h_b2, {C});
        maa::WeightStore ws(ctx->c.dtype != 0);
        maa::Ctx& c = ctx->c;
        maa::PackedW pw1 = ws.pack_conv(s.sd, "w1", h_b1 ? "b1" : "", 1, k1), pw2;
        if (h_w2) pw2 = ws.pack_conv(s.sd, "w2", h_b2 ? "b2" : "", 1, k2);
        maa::run_sized(c, [&] {
            maa::T4 x = maa::alloc_t(c, B, 1, L, C), y = maa::alloc_t(c, B, 1, L, C);
            maa::launch_nchw_to_nhwc(c, d_x, B, C, L, x.p);
            if (accumulate) maa::launch_nchw_to_nhwc(c, d_out, B, C, L, y.p);
            if (h_w2) {      // a ResBlock1 step; the residual is x
                maa::T4 t1 = maa::alloc_t(c, B, 1, L, C);
                maa::mrf_pair(c, x, pw1, k1, d1, slope1, pw2, k2, d2, slope2, x.p, out_scale, accumulate, t1, y);
            } else {         // a ResBlock2 step
                maa::conv1d_same(c, x, pw1, k1, d1, slope1, x.p, out_scale, accumulate, y);
            }
            maa::launch_nhwc_to_nchw(c, y.p, B, C, L, d_out, C);
        });
        MAA_HIP(hipStreamSynchronize(c.stream));
    });
}

}  // extern "C"
