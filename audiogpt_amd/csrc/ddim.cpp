// Device-resident DDIM loop: S x { build UNet input, UNet forward (2B with CFG), CFG combine + x_{t-1} update }.
//
// Mirrors ldm/models/diffusion/ddim.py:118-166 (ddim_sampling) and :169-225 (p_sample_ddim) of the
// reference: the tools' call pattern (eta = 0, no mask) and, since round 4, the rest of sample()'s signature that is pure
// tensor arithmetic -- mask / x0 blending (:147-150), eta > 0 with the caller's noise (:210-225), the logged intermediates
// (:158-163); score correctors, quantisation, dropout noise and host callbacks stay out:
//   CFG batch order is [uncond ; cond] on x, t and context (:177-199)
//   concat conditioning is cat([x, c], dim=1) (ldm/models/diffusion/ddpm.py:1404-1406)
// Nothing returns to the host inside the loop: per-step scalars (t, a_t, a_prev, sqrt(1-a_t)) are rows of
// device tables copied into fixed slots, so every step launches the same kernels on the same addresses and
// the step can be captured once as a hipGraph and replayed.  The latent and the concat conditioning are staged in the
// context's own slab, so the captured step does not depend on the caller's buffers and is KEPT across sample() calls
// (Ctx::ddim_graph): a later call with the same model, shapes and guidance replays it without capturing again.
#include "models.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace maa {

namespace {

// What every device loop over the DDIM tables shares -- DDIM's sample() / decode() and PLMS: the checks of the arguments, the
// loop's device state in the context's slab (tables, step index, slots, UNet input and output, the latent's and the concat
// conditioning's copies, the hoisted embeddings), the context projection and the guided forward's arrangement.  The
// constructor uploads everything and sets the device step index to `start`; prepare() and forward() are the launches of a
// step up to the UNet's output.
struct Loop {
    Ctx& ctx;
    UNet& unet;
    const maa_ddim_args& a;
    bool concat, cfg, masked, logging, emb_hoist, share, split;
    int nB, Cin;
    int crops, rows;                // split_input_params: crops per sample (1 without), UNet rows per step = nB * crops
    long long per_crop, per_crop_in;      // elements of one crop row of the UNet's output / input
    long long per, per_in;          // latent elements per sample, UNet input elements per sample
    size_t emb_w;
    std::vector<float> h_tab;       // (h_tab, h_wT and h_step are read by async copies: they live until the loop's final synchronisation)
    std::vector<float> h_wT;        // the split's weighting transposed, [L][kh * kw]
    int h_step;
    float *slab, *tab_t, *tab_coef, *cur_t, *cur_coef, *xin, *eps, *xs, *ccs, *emb_tab, *cur_emb;
    float *wT = nullptr, *norm = nullptr, *zin = nullptr, *ecrop = nullptr;      // split: weighting, its fold, crop input, crop eps
    int* d_step;
    Ctx* lane2;

    Loop(Ctx& ctx_, UNet& unet_, const maa_ddim_args& a_, int start, const float* d_x) : ctx(ctx_), unet(unet_), a(a_) {
        MAA_CHECK(!a.d_uncond || a.d_cond, "ddim: unconditional conditioning given without conditioning");
        MAA_CHECK(!a.d_cond || a.L > 0, "ddim: conditioning needs its token count L");
        MAA_CHECK(!a.d_concat || a.Cc > 0, "ddim: concat conditioning needs its channel count");
        concat = a.d_concat != nullptr;
        cfg = !concat && a.d_uncond != nullptr && a.scale != 1.0f;
        nB = cfg ? 2 * a.B : a.B;
        Cin = concat ? a.C + a.Cc : a.C;
        per = (long long)a.C * a.H * a.W;
        per_in = (long long)Cin * a.H * a.W;
        MAA_CHECK(unet.config().in_channels == Cin, "ddim: UNet in_channels does not match latent (+concat) channels");
        // split_input_params (ddpm_audio.py:572-654): every model evaluation runs on overlapping crops of the latent
        split = a.split_kh != 0 || a.split_kw != 0 || a.split_sh != 0 || a.split_sw != 0 || a.h_split_weight != nullptr;
        MAA_CHECK(!split || (a.split_kh > 0 && a.split_kw > 0 && a.split_sh > 0 && a.split_sw > 0 && a.h_split_weight),
                  "ddim: the split needs ks, stride and the weighting (all zero / NULL: no split)");
        MAA_CHECK(!split || !concat, "ddim: a concat-conditioned model cannot be split (every crop would get the full-size concat tensor)");
        crops = split ? split_crops(a.H, a.W, a.split_kh, a.split_kw, a.split_sh, a.split_sw) : 1;
        rows = nB * crops;
        per_crop = split ? (long long)a.C * a.split_kh * a.split_kw : per;
        per_crop_in = split ? (long long)Cin * a.split_kh * a.split_kw : per_in;

        // ---- device state of the loop, in one slab the context keeps across calls: tables (one row per DDIM index), the
        // device step index, the step's timestep / coefficient slots, UNet input and output
        masked = a.d_mask != nullptr;
        MAA_CHECK(!masked || (a.d_x0 && a.d_noise_q && a.h_sqrt_ac && a.h_sqrt_1mac), "ddim: mask needs x0, its noise and the q_sample tables");
        MAA_CHECK(!a.h_sigmas || a.d_noise_p, "ddim: eta > 0 needs the steps' noise");
        // (noise_p itself may point before the caller's buffer -- decode's offset -- so it is tested through a.d_noise_p only)
        logging = a.n_log > 0;
        MAA_CHECK(!logging || (a.d_log_x && a.d_log_x0 && a.log_every_t > 0), "ddim: intermediates need their buffers and log_every_t");
        h_tab.assign((size_t)a.S * 9, 0.f);
        int n_logged = 0;
        for (int v = 0; v < a.S; ++v) {                    // visiting order: index S-1 first (ddim.py:143-145)
            const int i = a.S - 1 - v;
            h_tab[i] = (float)a.h_timesteps[i];
            float* cf = &h_tab[(size_t)a.S + (size_t)i * 8];
            cf[0] = a.h_alphas[i];
            cf[1] = a.h_alphas_prev[i];
            cf[2] = a.h_sigmas ? a.h_sigmas[i] : 0.f;      // eta = 0: no noise term
            cf[3] = std::sqrt(1.0f - a.h_alphas[i]);       // ddim.py:52 (fp32 sqrt of fp32 1-a)
            cf[4] = masked ? a.h_sqrt_ac[i] : 0.f;
            cf[5] = masked ? a.h_sqrt_1mac[i] : 0.f;
            const bool logged = logging && (i % a.log_every_t == 0 || i == a.S - 1);      // ddim.py:161
            cf[6] = logged ? (float)n_logged++ : -1.f;
            cf[7] = (float)i;
        }
        MAA_CHECK(!logging || n_logged == a.n_log, "ddim: n_log does not match log_every_t");
        auto up = [](size_t n) { return (n + 63) / 64 * 64; };      // floats, 256-byte aligned pieces
        const size_t n_cc = concat ? (size_t)a.B * (per_in - per) : 0;
        // the ResBlocks' time-embedding rows of all S steps, computed once per call (every sample of a step shares t; the I2A
        // variant adds the sample's context to the embedding and keeps the per-forward computation): six launches leave every step
        emb_hoist = !unet.config().add_context_to_emb;
        emb_w = emb_hoist ? (size_t)unet.emb_width() : 0;
        // (the split's pieces follow the others: the weighting, its fold, the crop rows of the UNet's input and output; the
        // timestep slots hold one per crop row)
        const size_t kk = split ? (size_t)a.split_kh * a.split_kw : 0;
        const size_t o_tab = 0, o_step = o_tab + up(h_tab.size()), o_t = o_step + 64, o_coef = o_t + up(rows),
                     o_xin = o_coef + 64, o_eps = o_xin + up((size_t)nB * per_in), o_x = o_eps + up((size_t)nB * per),
                     o_cc = o_x + up((size_t)a.B * per), o_embt = o_cc + up(n_cc), o_emb = o_embt + up((size_t)a.S * emb_w),
                     o_wT = o_emb + up(emb_w), o_norm = o_wT + up(kk * crops), o_zin = o_norm + up(split ? (size_t)a.H * a.W : 0),
                     o_ecrop = o_zin + up(split ? (size_t)rows * per_crop_in : 0),
                     total = o_ecrop + up(split ? (size_t)rows * per_crop : 0);
        slab = static_cast<float*>(ctx.sampler_scratch.get(total * sizeof(float), ctx.stream));
        if (split) {
            wT = slab + o_wT, norm = slab + o_norm, zin = slab + o_zin, ecrop = slab + o_ecrop;
            h_wT = split_weight_transposed(a.h_split_weight, kk, crops);
            MAA_HIP(hipMemcpyAsync(wT, h_wT.data(), h_wT.size() * 4, hipMemcpyHostToDevice, ctx.stream));
            launch_split_norm(ctx, wT, a.H, a.W, a.split_kh, a.split_kw, a.split_sh, a.split_sw, norm);
        }
        tab_t = slab + o_tab, tab_coef = slab + o_tab + a.S, cur_t = slab + o_t, cur_coef = slab + o_coef, xin = slab + o_xin,
        eps = slab + o_eps, xs = slab + o_x, ccs = slab + o_cc, emb_tab = slab + o_embt, cur_emb = slab + o_emb;
        // the trajectory runs on the slab's copy of the latent (and of the concat conditioning)
        MAA_HIP(hipMemcpyAsync(xs, d_x, (size_t)a.B * per * 4, hipMemcpyDeviceToDevice, ctx.stream));
        if (concat) MAA_HIP(hipMemcpyAsync(ccs, a.d_concat, n_cc * 4, hipMemcpyDeviceToDevice, ctx.stream));
        d_step = reinterpret_cast<int*>(slab + o_step);
        MAA_HIP(hipMemcpyAsync(slab + o_tab, h_tab.data(), h_tab.size() * 4, hipMemcpyHostToDevice, ctx.stream));
        h_step = start;                                  // ddim.py:143-145: flipped timesteps, index = total - i - 1
        MAA_HIP(hipMemcpyAsync(d_step, &h_step, 4, hipMemcpyHostToDevice, ctx.stream));

        if (emb_hoist) unet.emb_table(ctx, tab_t, a.S, emb_tab);      // (tab_t: the S timesteps as floats, uploaded above)

        // ---- conditioning: constant over the trajectory -> project K/V once (split: once per sample, served to its crops)
        if (!concat && a.d_cond) {
            if (cfg)
                unet.set_context_cfg(ctx, a.d_uncond, a.d_cond, a.B, a.L, crops);
            else
                unet.set_context(ctx, a.d_cond, nB, a.L, crops);
        }

        // Classifier-free guidance: the reference evaluates the model once on cat([x] * 2) (ddim.py:177-199); the two halves are
        // independent until the combine, and one batch of 8 prompts leaves much of the chip idle, so the step
        // forks after the UNet input is built -- the unconditional half on the context's stream, the conditional half on the
        // second lane's stream and workspace -- and joins before the update kernel.  Captured, the halves are two branches of the
        // step graph.  Every kernel is batch-invariant bit for bit, so the result equals the one-stream form's.
        const bool two_lanes = cfg && ctx.split_cfg();
        lane2 = two_lanes ? &side_lane(ctx) : nullptr;
        if (lane2 && ctx.prof && !lane2->prof) {
            lane2->prof = new Profiler;
            lane2->prof->detail = ctx.prof->detail;
        }
        // a guided step's halves are the same tensor up to the first cross-attention: computed once (MAA_CFG_SHARED=0: twice)
        share = cfg && emb_hoist && ctx.tune.cfg_shared;
    }

    // the step's UNet input (cat([x] * 2) / cat([x, c]), the mask blend) and its timestep / coefficient / embedding slots
    void prepare() {
        launch_ddim_prepare(ctx, xs, concat ? ccs : nullptr, a.B, nB, per, per_in - per, tab_t, tab_coef, d_step, xin, cur_t,
                            cur_coef, a.d_mask, a.d_x0, a.d_noise_q, a.S, emb_hoist ? emb_tab : nullptr, (int)emb_w, cur_emb, rows);
    }

    // eps = UNet(xin, cur_t) over nB rows (with CFG: [uncond ; cond], on one stream or as two lanes).  With the split the UNet
    // runs over the nB * crops crop rows of xin -- unfold keeps each half's rows together, so the halves, the shared prefix and
    // the lanes are what they are without it -- and fold stitches its output into eps.
    void forward() {
        const float* in = xin;
        float* out = eps;
        int h = a.H, w = a.W;
        if (split) {
            launch_split_unfold(ctx, xin, nB, Cin, a.H, a.W, a.split_kh, a.split_kw, a.split_sh, a.split_sw, zin);
            in = zin, out = ecrop, h = a.split_kh, w = a.split_kw;
        }
        const int half = a.B * crops;      // UNet rows of one half of a guided step
        const float* emb_row = emb_hoist ? cur_emb : nullptr;
        if (lane2) {
            MAA_HIP(hipEventRecord(ctx.ev_fork, ctx.stream));
            MAA_HIP(hipStreamWaitEvent(lane2->stream, ctx.ev_fork, 0));
            // (the conditional lane starts from the unconditional lane's layers before the first cross-attention: this call's
            // hand-over, filled by the first forward and read by the second)
            CfgPrefix handover;
            handover.ready = ctx.ev_prefix;
            UNetForwardOpt o{emb_row, 0, share ? CfgShare::Export : CfgShare::None, &handover};
            unet.forward(ctx, in, cur_t, unet.context_ptr, half, h, w, out, o);
            o.batch_off = half, o.mode = share ? CfgShare::Import : CfgShare::None;
            unet.forward(*lane2, in + (size_t)half * per_crop_in, cur_t + half, unet.context_ptr, half, h, w,
                         out + (size_t)half * per_crop, o);
            MAA_HIP(hipEventRecord(ctx.ev_join, lane2->stream));
            MAA_HIP(hipStreamWaitEvent(ctx.stream, ctx.ev_join, 0));
        } else
            // (one stream: the halves of cat([x] * 2) share every layer before the first cross-attention)
            unet.forward(ctx, in, cur_t, unet.context_ptr, rows, h, w, out, {emb_row, -1, share ? CfgShare::Dup : CfgShare::None, nullptr});
        if (split)
            launch_split_fold(ctx, ecrop, wT, norm, nB, a.C, a.H, a.W, a.split_kh, a.split_kw, a.split_sh, a.split_sw, eps);
    }

    // the loop's tail: the slab's latent back to the caller's, synchronised (the host tables go out of scope; the call returns a
    // finished latent)
    void finish(float* d_x) {
        MAA_HIP(hipMemcpyAsync(d_x, xs, (size_t)a.B * per * 4, hipMemcpyDeviceToDevice, ctx.stream));
        MAA_HIP(hipStreamSynchronize(ctx.stream));
    }

    // Everything a captured step depends on besides the device-side state it reads: the model and its own buffers, the
    // shapes, the guidance scale, the slab (every slot's offset is a function of the numbers listed) and the workspace.
    // (The workspace base / capacity go in AFTER the first eager step, which may grow it.)
    std::vector<unsigned long long> key(const float* noise_p) const {
        std::vector<unsigned long long> k;
        unet.graph_key(k);
        unsigned scale_bits, temp_bits;
        static_assert(sizeof(scale_bits) == sizeof(a.scale), "float bits");
        std::memcpy(&scale_bits, &a.scale, 4);
        std::memcpy(&temp_bits, &a.temperature, 4);
        k.push_back(temp_bits);
        for (unsigned long long v : {(unsigned long long)a.S, (unsigned long long)a.B, (unsigned long long)a.C, (unsigned long long)a.H,
                                     (unsigned long long)a.W, (unsigned long long)a.Cc, (unsigned long long)a.L,
                                     (unsigned long long)cfg, (unsigned long long)concat, (unsigned long long)scale_bits,
                                     (unsigned long long)ctx.dtype, (unsigned long long)reinterpret_cast<uintptr_t>(slab),
                                     // the caller's buffers the step's launches read or write besides the slab
                                     (unsigned long long)reinterpret_cast<uintptr_t>(a.d_mask),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(a.d_x0),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(a.d_noise_q),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(a.h_sigmas ? noise_p : nullptr),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(logging ? a.d_log_x : nullptr),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(logging ? a.d_log_x0 : nullptr),
                                     (unsigned long long)(a.h_sigmas ? 1 : 0),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(ctx.stream),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(ctx.ws.base()),
                                     (unsigned long long)ctx.ws.capacity(),
                                     // the second lane of a CFG step: its stream and workspace are part of the captured step
                                     (unsigned long long)reinterpret_cast<uintptr_t>(lane2 ? lane2->stream : nullptr),
                                     (unsigned long long)reinterpret_cast<uintptr_t>(lane2 ? lane2->ws.base() : nullptr),
                                     (unsigned long long)(lane2 ? lane2->ws.capacity() : 0),
                                     // the guided step's arrangement: the shared prefix changes the launches, as the lanes do
                                     (unsigned long long)share, (unsigned long long)(lane2 != nullptr),
                                     // the split: a step with it launches other kernels on other shapes than one without
                                     (unsigned long long)a.split_kh, (unsigned long long)a.split_kw, (unsigned long long)a.split_sh,
                                     (unsigned long long)a.split_sw, (unsigned long long)reinterpret_cast<uintptr_t>(wT)})
            k.push_back(v);
        return k;
    }
};

// The loop body of sample() and decode(): n_steps steps of the S-step schedule `a` describes, from DDIM index `start` down to
// start - n_steps + 1.  sample() is (S - 1, S); decode(t_start) is (t_start - 1, t_start).  The start only sets the device step
// index before the first step, so it is not part of the step graph's key: a decode with the same S, shapes, guidance and buffers
// as the last sample replays the kept graph.  noise_p: the pointer the step kernel indexes as noise_p + (S - 1 - idx) * n.
void ddim_run(Ctx& ctx, UNet& unet, const maa_ddim_args& a, int start, int n_steps, const float* noise_p, float* d_x) {
    MAA_CHECK(a.S > 0 && a.B > 0, "ddim: empty problem");
    MAA_CHECK(start >= 0 && start < a.S && n_steps > 0 && n_steps <= start + 1, "ddim: steps outside the schedule");
    Loop lp(ctx, unet, a, start, d_x);

    // one step: identical launches on identical addresses whatever the step (the index lives on the device)
    auto step_body = [&]() {
        lp.prepare();
        lp.forward();
        launch_ddim_step(ctx, lp.xin, lp.per, lp.per_in, lp.eps, lp.cfg ? lp.eps + a.B * lp.per : nullptr, a.scale, lp.cur_coef,
                         (long long)a.B * lp.per, lp.xs, a.h_sigmas ? noise_p : nullptr, a.temperature, a.S,
                         lp.logging ? a.d_log_x : nullptr, lp.logging ? a.d_log_x0 : nullptr, lp.d_step);
    };

    run_steps(ctx, ctx.ddim_graph, n_steps, a.use_graph != 0, false, [&] { return lp.key(noise_p); }, step_body,
              [&](int i, char* buf, size_t len) { std::snprintf(buf, len, "ddim_step %d/%d t=%d", i + 1, n_steps, (int)a.h_timesteps[start - i]); });
    lp.finish(d_x);
}

}  // namespace

void ddim_sample(Ctx& ctx, UNet& unet, const maa_ddim_args& a, float* d_x) { ddim_run(ctx, unet, a, a.S - 1, a.S, a.d_noise_p, d_x); }

// ---- The argument checks of the entry points below that touch no device: api.cpp runs them before it binds the context, so a
// malformed call fails the same way with or without a device; the functions they guard do not repeat them.
void check_ddim_decode_args(const void* unet, const maa_ddim_args* a, int t_start, const float* d_x) {
    MAA_CHECK(unet && a && d_x && a->h_timesteps && a->h_alphas && a->h_alphas_prev, "bad ddim_decode arguments");
    MAA_CHECK(a->S > 0 && a->B > 0, "bad ddim_decode arguments: empty problem");
    MAA_CHECK(t_start >= 0 && t_start <= a->S, "bad ddim_decode arguments: t_start must lie in [0, S]");
    MAA_CHECK(!a->d_mask && !a->d_x0 && !a->d_noise_q && !a->h_sqrt_ac && !a->h_sqrt_1mac,
              "bad ddim_decode arguments: decode takes no mask / x0 (ddim.py:243-245)");
    MAA_CHECK(a->n_log == 0 && !a->d_log_x && !a->d_log_x0, "bad ddim_decode arguments: decode logs no intermediates");
}
void check_ldm_plms_args(const void* unet, const maa_ddim_args* a, const float* d_x) {
    MAA_CHECK(unet && a && d_x && a->h_timesteps && a->h_alphas && a->h_alphas_prev, "bad ldm_plms_sample arguments");
    MAA_CHECK(a->S > 0 && a->B > 0, "bad ldm_plms_sample arguments: empty problem");
    MAA_CHECK(!a->h_sigmas && !a->d_noise_p,
              "bad ldm_plms_sample arguments: ddim_eta must be 0 for PLMS (h_sigmas and d_noise_p must be NULL)");
}
void check_ddpm_sample_args(const void* unet, const maa_ddpm_args* a, const float* d_x) {
    MAA_CHECK(unet && a && d_x, "bad ddpm_sample arguments: null pointer");
    const maa_ddim_args& l = a->loop;
    MAA_CHECK(l.S > 0 && l.B > 0 && l.C > 0 && l.H > 0 && l.W > 0, "bad ddpm_sample arguments: empty problem");
    MAA_CHECK(a->n >= 1 && a->n <= l.S, "bad ddpm_sample arguments: the number of steps must lie in 1 .. num_timesteps");
    MAA_CHECK(a->start >= a->n - 1 && a->start < l.S, "bad ddpm_sample arguments: steps outside the schedule");
    MAA_CHECK(a->h_sqrt_recip_ac && a->h_sqrt_recipm1_ac && a->h_coef1 && a->h_coef2 && a->h_logvar,
              "bad ddpm_sample arguments: the posterior tables are missing");
    MAA_CHECK(l.d_noise_p, "bad ddpm_sample arguments: the steps' noise is missing");
    MAA_CHECK(!l.d_mask || (l.d_x0 && l.d_noise_q && a->h_sqrt_ac && a->h_sqrt_1mac),
              "bad ddpm_sample arguments: mask needs x0, its noise and the q_sample tables");
    if (l.n_log > 0 || l.d_log_x || l.d_log_x0) {
        MAA_CHECK(l.d_log_x && l.d_log_x0 && l.log_every_t > 0, "bad ddpm_sample arguments: intermediates need their buffers and log_every_t");
        int n_logged = 0;      // ddpm_audio.py:877 with timesteps - 1 = the first step run
        for (int t = a->start; t > a->start - a->n; --t) n_logged += (t % l.log_every_t == 0 || t == a->start);
        MAA_CHECK(n_logged == l.n_log, "bad ddpm_sample arguments: n_log does not match log_every_t");
    }
}
void check_ddpm_update_args(const float* d_x, const float* d_eps, const int32_t* d_t, const float* h_sqrt_recip_ac,
                            const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_logvar, int n_tab,
                            const float* d_noise, int B, int C, int H, int W, const float* d_x_prev, const float* d_x_recon) {
    MAA_CHECK(d_x && d_eps && d_t && d_noise && d_x_prev && d_x_recon, "bad ddpm_update arguments: null pointer");
    MAA_CHECK(h_sqrt_recip_ac && h_sqrt_recipm1_ac && h_coef1 && h_coef2 && h_logvar, "bad ddpm_update arguments: the posterior tables are missing");
    MAA_CHECK(B > 0 && C > 0 && H > 0 && W > 0 && n_tab > 0, "bad ddpm_update arguments: empty shape or table");
    for (const float* out : {d_x_prev, d_x_recon})
        MAA_CHECK(out != d_x && out != d_eps && out != d_noise, "bad ddpm_update arguments: the outputs may not alias the inputs");
    MAA_CHECK(d_x_prev != d_x_recon, "bad ddpm_update arguments: the outputs may not alias each other");
}
void check_stochastic_encode_args(const float* d_x0_or_moments, bool from_moments, const float* d_noise_post, const int32_t* d_t,
                                  const float* h_sqrt_a, const float* h_sqrt_1ma, int n_tab, const float* d_noise, int B, int C, int H,
                                  int W, const float* d_out) {
    MAA_CHECK(d_x0_or_moments && d_t && h_sqrt_a && h_sqrt_1ma && d_noise && d_out, "bad stochastic_encode arguments: null pointer");
    MAA_CHECK(B > 0 && C > 0 && H > 0 && W > 0 && n_tab > 0, "bad stochastic_encode arguments: empty shape or table");
    MAA_CHECK(!from_moments || d_noise_post, "bad stochastic_encode arguments: the moments need their posterior noise");
}

// ddim.py:243-261: decode runs p_sample_ddim over timesteps[:t_start] flipped, i.e. DDIM indices t_start - 1 .. 0 with the tables
// of the whole schedule -- the tail of sample()'s loop.  Its caller's noise holds t_start draws (first step first); the step kernel
// reads draw S - 1 - idx of its pointer, so the pointer handed over starts S - t_start draws before the caller's buffer (only
// draws S - t_start .. S - 1 of it, the caller's 0 .. t_start - 1, are ever read).
void ddim_decode(Ctx& ctx, UNet& unet, const maa_ddim_args& a, int t_start, float* d_x) {
    if (t_start == 0) return;                          // the reference's loop is empty: x_latent comes back unchanged
    const float* noise_p = nullptr;
    if (a.h_sigmas && a.d_noise_p) {
        const long long n = (long long)a.B * a.C * a.H * a.W;
        noise_p = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(a.d_noise_p) -
                                                 (uintptr_t)((long long)(a.S - t_start) * n * (long long)sizeof(float)));
    }
    ddim_run(ctx, unet, a, t_start - 1, t_start, noise_p, d_x);
}

// PLMSSampler.plms_sampling + p_sample_plms (plms.py:115-236) on the DDIM loop's state (Loop above) with sigma = 0 (the
// reference's noise draws are multiplied by it; the caller makes them) and a ring of three e_t slabs (ldm_plms_* in sampler_steps.hip):
//   step 0 (no history): prepare, eps(x, t), Euler mid-point kernel (e_t -> ring slot 0, the blended x -> the latent slab,
//     x_mid -> the UNet input, t / embedding slots -> t_next), eps(x_mid, t_next), final kernel (update with (e_t + e_next) / 2);
//   steps 1 .. S-1: prepare, eps(x, t), one kernel (Adams-Bashforth over the ring, update, logs).
// Step 0 runs eager (its two forwards size the workspace); the Adams-Bashforth step is captured once into Ctx::plms_graph and
// replayed: its launches are the same for every step (the ring slot and the order follow from the device index).  The graph is
// kept across calls under the DDIM loop's key plus the ring's address, apart from the DDIM graph.
void ldm_plms_sample(Ctx& ctx, UNet& unet, const maa_ddim_args& a, float* d_x) {
    Loop lp(ctx, unet, a, a.S - 1, d_x);
    const long long n = (long long)a.B * lp.per;
    float* ring = static_cast<float*>(ctx.plms_ring.get((size_t)3 * n * sizeof(float), ctx.stream));
    const float* eps_c = lp.cfg ? lp.eps + n : nullptr;
    float* log_x = lp.logging ? a.d_log_x : nullptr;
    float* log_x0 = lp.logging ? a.d_log_x0 : nullptr;

    auto euler_step = [&]() {
        lp.prepare();
        lp.forward();
        launch_ldm_plms_euler_mid(ctx, lp.xin, lp.per, lp.per_in, a.B, lp.nB, lp.eps, eps_c, a.scale, lp.cur_coef, lp.xs, ring,
                                  lp.tab_t, lp.cur_t, lp.emb_hoist ? lp.emb_tab : nullptr, (int)lp.emb_w, lp.cur_emb, lp.rows);
        lp.forward();
        launch_ldm_plms_euler_final(ctx, lp.eps, eps_c, a.scale, lp.cur_coef, n, lp.xs, ring, log_x, log_x0, lp.d_step);
    };
    auto ab_step = [&]() {
        lp.prepare();
        lp.forward();
        launch_ldm_plms_step(ctx, lp.xin, lp.per, lp.per_in, lp.eps, eps_c, a.scale, lp.cur_coef, n, lp.xs, ring, a.S, log_x, log_x0,
                             lp.d_step);
    };
    auto key = [&]() {
        std::vector<unsigned long long> k = lp.key(nullptr);
        k.push_back((unsigned long long)reinterpret_cast<uintptr_t>(ring));
        return k;
    };

    MAA_RANGE_PUSH("plms_step 1 (Euler pair)");
    euler_step();
    MAA_RANGE_POP();
    // (the Euler pair has sized the workspace; the runner's step i is the loop's step i + 1)
    run_steps(ctx, ctx.plms_graph, a.S - 1, a.use_graph != 0, true, key, ab_step,
              [&](int i, char* buf, size_t len) { std::snprintf(buf, len, "plms_step %d/%d t=%d", i + 2, a.S, (int)a.h_timesteps[a.S - 2 - i]); });
    lp.finish(d_x);
}

// LatentDiffusion_audio's ancestral chain (ddpm_audio.py:717-884: p_mean_variance, p_sample, p_sample_loop, progressive_denoising)
// on the DDIM loop's state: the "schedule" Loop sees is the identity over the model's T DDPM timesteps (index = timestep, so the
// hoisted embeddings are those of t = 0 .. T-1 whatever part of the chain a call runs), without mask, noise or logs -- those
// belong to the step kernel here, which blends AFTER the update and reads its coefficients from a table of its own (Ctx::ddpm_tab,
// one row per timestep) by the index in the step's coefficient slot.  Steps t = start .. start - n + 1; the first runs eager (it
// sizes the workspace), then one step is captured into Ctx::ddpm_graph and replayed, kept across calls under the loop's key plus
// everything the step kernel is launched with.
void ddpm_sample(Ctx& ctx, UNet& unet, const maa_ddpm_args& a, float* d_x) {
    const maa_ddim_args& u = a.loop;
    const int T = u.S;
    const bool masked = u.d_mask != nullptr;
    const bool logging = u.n_log > 0;

    // nonzero_mask * (0.5 * model_log_variance).exp(), fp32 as torch's
    std::vector<float> h_tab = posterior_rows(a.h_sqrt_recip_ac, a.h_sqrt_recipm1_ac, a.h_coef1, a.h_coef2, T,
                                              [&](int t) { return std::exp(0.5f * a.h_logvar[t]); }, DDPM_TAB_W);
    for (int t = 0; t < T; ++t) {
        float* r = &h_tab[(size_t)t * DDPM_TAB_W];
        r[5] = a.h_temperature ? a.h_temperature[t] : 1.f;
        r[6] = masked ? a.h_sqrt_ac[t] : 0.f;
        r[7] = masked ? a.h_sqrt_1mac[t] : 0.f;
        r[8] = -1.f;
    }
    int n_logged = 0;
    for (int t = a.start; t > a.start - a.n; --t)                   // ddpm_audio.py:877 with timesteps - 1 = the first step run
        if (logging && (t % u.log_every_t == 0 || t == a.start)) h_tab[(size_t)t * DDPM_TAB_W + 8] = (float)n_logged++;

    // what Loop sees: the identity schedule, no blend before the step, no noise term, no logs of its own
    std::vector<int32_t> h_ts((size_t)T);
    std::vector<float> h_one((size_t)T, 1.0f);
    for (int t = 0; t < T; ++t) h_ts[t] = t;
    maa_ddim_args la = u;
    la.h_timesteps = h_ts.data(), la.h_alphas = la.h_alphas_prev = h_one.data();
    la.d_mask = la.d_x0 = la.d_noise_q = la.d_noise_p = nullptr;
    la.h_sqrt_ac = la.h_sqrt_1mac = la.h_sigmas = nullptr;
    la.temperature = 1.0f;
    la.log_every_t = la.n_log = 0;
    la.d_log_x = la.d_log_x0 = nullptr;
    Loop lp(ctx, unet, la, a.start, d_x);

    float* tab = static_cast<float*>(ctx.ddpm_tab.get(h_tab.size() * sizeof(float), ctx.stream));
    MAA_HIP(hipMemcpyAsync(tab, h_tab.data(), h_tab.size() * sizeof(float), hipMemcpyHostToDevice, ctx.stream));
    const long long nel = (long long)u.B * lp.per;
    float* log_x = logging ? u.d_log_x : nullptr;
    float* log_x0 = logging ? u.d_log_x0 : nullptr;
    auto step_body = [&]() {
        lp.prepare();
        lp.forward();
        launch_ddpm_step(ctx, lp.xin, lp.per, lp.per_in, lp.eps, lp.cfg ? lp.eps + nel : nullptr, u.scale, lp.cur_coef, tab, nel, lp.xs,
                         u.d_noise_p, a.start, a.clip_denoised != 0, u.d_mask, u.d_x0, u.d_noise_q, log_x, log_x0, lp.d_step);
    };
    auto key = [&]() {
        std::vector<unsigned long long> k = lp.key(nullptr);
        for (const void* p : {(const void*)tab, (const void*)u.d_noise_p, (const void*)u.d_mask, (const void*)u.d_x0,
                              (const void*)u.d_noise_q, (const void*)log_x, (const void*)log_x0})
            k.push_back((unsigned long long)reinterpret_cast<uintptr_t>(p));
        k.push_back((unsigned long long)a.start);
        k.push_back((unsigned long long)(a.clip_denoised != 0));
        return k;
    };
    run_steps(ctx, ctx.ddpm_graph, a.n, u.use_graph != 0, false, key, step_body,
              [&](int i, char* buf, size_t len) { std::snprintf(buf, len, "ddpm_step %d/%d t=%d", i + 1, a.n, a.start - i); });
    lp.finish(d_x);
}

// p_sample's arithmetic for one step (ddpm_audio.py:748-777) with a timestep per sample: the five tables go up next to an error
// flag in a slab of their own, as ddim_stochastic_encode's do.
void ddpm_update(Ctx& ctx, const float* d_x, const float* d_eps, const int32_t* d_t, const float* h_sqrt_recip_ac,
                 const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_logvar, int n_tab,
                 const float* d_noise, float temperature, bool clip, int B, int C, int H, int W, float* d_x_prev, float* d_x_recon) {
    FlaggedTable ft(ctx, ctx.ddpm_scratch, posterior_rows(h_sqrt_recip_ac, h_sqrt_recipm1_ac, h_coef1, h_coef2, n_tab,
                                                         [&](int t) { return std::exp(0.5f * h_logvar[t]); }));
    launch_ddpm_update(ctx, d_x, d_eps, d_t, ft.tab, n_tab, d_noise, temperature, clip, B, (long long)C * H * W, d_x_prev, d_x_recon,
                       ft.bad);
    ft.check("ddpm_update: some t[b] lies outside [0, n_tab)");
}

// One evaluation of the model with split_input_params (ddpm_audio.py:572-654) outside a loop: what Loop::forward does per step,
// on the caller's x / t / context.  Its device state lives in the context's split_scratch: [wT | norm | crop input | crop eps | t].
void unet_forward_split(Ctx& ctx, UNet& unet, const float* d_x, const float* d_t, const float* d_context, int B, int H, int W, int kh,
                        int kw, int sh, int sw, const float* h_weight, float* d_out) {
    const maa_unet_config& uc = unet.config();
    const int L = split_crops(H, W, kh, kw, sh, sw);
    const size_t kk = (size_t)kh * kw;
    const long long rows = (long long)B * L;
    MAA_CHECK(rows <= (1 << 20), "forward_split: too many crop rows");
    if (uc.use_spatial_transformer) {
        MAA_CHECK(d_context && unet.context_len() > 0,
                  "forward_split: this UNet needs d_context, [B, L, context_dim] with the token count L of an earlier maa_unet_set_context");
        unet.set_context(ctx, d_context, B, unet.context_len(), L);
    }
    auto up = [](size_t n) { return (n + 63) / 64 * 64; };
    const size_t o_wT = 0, o_norm = o_wT + up(kk * L), o_zin = o_norm + up((size_t)H * W),
                 o_e = o_zin + up((size_t)rows * uc.in_channels * kk), o_t = o_e + up((size_t)rows * uc.out_channels * kk),
                 total = o_t + up((size_t)rows);
    float* slab = static_cast<float*>(ctx.split_scratch.get(total * sizeof(float), ctx.stream));
    const std::vector<float> h_wT = split_weight_transposed(h_weight, kk, L);
    MAA_HIP(hipMemcpyAsync(slab + o_wT, h_wT.data(), h_wT.size() * 4, hipMemcpyHostToDevice, ctx.stream));
    MAA_HIP(hipStreamSynchronize(ctx.stream));      // (h_wT goes out of scope; everything after is asynchronous)
    launch_split_norm(ctx, slab + o_wT, H, W, kh, kw, sh, sw, slab + o_norm);
    launch_repeat_rows(ctx, d_t, B, 1, L, slab + o_t);
    launch_split_unfold(ctx, d_x, B, uc.in_channels, H, W, kh, kw, sh, sw, slab + o_zin);
    unet.forward(ctx, slab + o_zin, slab + o_t, unet.context_ptr, (int)rows, kh, kw, slab + o_e);
    launch_split_fold(ctx, slab + o_e, slab + o_wT, slab + o_norm, B, uc.out_channels, H, W, kh, kw, sh, sw, d_out);
}

// ddim.py:227-241.  The two coefficient tables, A (n_tab) then B (n_tab), go up once per call next to an error flag in the context's
// own slab; the flag is read back after the launch (the call synchronises the stream: the host tables and the caller's t are its inputs).
void ddim_stochastic_encode(Ctx& ctx, const float* d_x0_or_moments, bool from_moments, float scale_factor, const float* d_noise_post,
                            const int32_t* d_t, const float* h_sqrt_a, const float* h_sqrt_1ma, int n_tab, const float* d_noise, int B,
                            int C, int H, int W, float* d_out) {
    std::vector<float> h_tab(h_sqrt_a, h_sqrt_a + n_tab);
    h_tab.insert(h_tab.end(), h_sqrt_1ma, h_sqrt_1ma + n_tab);
    FlaggedTable ft(ctx, ctx.encode_scratch, std::move(h_tab));
    launch_ddim_stochastic_encode(ctx, from_moments ? nullptr : d_x0_or_moments, from_moments ? d_x0_or_moments : nullptr,
                                  scale_factor, from_moments ? d_noise_post : nullptr, d_t, ft.tab, n_tab, d_noise, B,
                                  (long long)C * H * W, d_out, ft.bad);
    ft.check("stochastic_encode: some t[b] lies outside [0, n_tab)");
}

}  // namespace maa
