// DiffSinger's denoiser (DiffNet) and its two sampling loops on the device (the T2S tool's diffusion hot
// loop, audio-chatgpt.py:298-339).
//
// Mirrors NeuralSeq/modules/diff/net.py:58-130 (ResidualBlock, DiffNet.forward) and
// NeuralSeq/modules/diff/shallow_diffusion_tts.py:166-201, 262-269 (p_sample_plms and its loop with pndm_speedup) and
// :134-166, 269-271 (p_sample and the ancestral loop every configuration without pndm_speedup takes).
// Layout: channels-last sequences [B, T, C]; a Conv1d(k = 1) is a plain GEMM over the B*T rows, the dilated k = 3 conv an
// implicit GEMM.  Differences from a literal translation (same maths):
//   * the 20 per-layer `diffusion_projection` Linears of the step embedding run as ONE GEMM per evaluation
//   * the 20 per-layer `conditioner_projection` convs of the (step-invariant) conditioning run ONCE per sample() call,
//     as one GEMM, and enter each layer's dilated conv as its residual epilogue
//   * relu, bias, the conditioner add and 1/sqrt(n_layers) are igemm epilogues; the gate, the residual/skip update and
//     the next layer's `x + step` are two elementwise kernels per layer
//   * the sampling loop keeps t, the noise-history ring and its fill count on the device, so every step after the
//     first is the same launch sequence: captured once as a hipGraph and replayed
#include "models.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace maa {

struct DiffNet::Impl {
    maa_diffnet_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    PackedW in_proj, mlp0, mlp2, step_all, cond_all, skip_proj, out_proj;
    std::vector<PackedW> dilated, out_layer;
    DevSlab cond_cache;       // conditioner projections of all layers for the current conditioning: [B*T, L * 2C]
    const float* cond_src = nullptr;
    int cond_B = 0, cond_T = 0;
    DevSlab loop;             // state of the sampling loop that runs (PLMS or ancestral; each call writes all of its own)

    void build(const StateDict& sd) {
        const int L = cfg.residual_layers;
        in_proj = ws.pack_conv(sd, "input_projection.weight", "input_projection.bias", 1, 1);
        mlp0 = ws.pack_conv(sd, "mlp.0.weight", "mlp.0.bias", 1, 1);
        mlp2 = ws.pack_conv(sd, "mlp.2.weight", "mlp.2.bias", 1, 1);
        std::vector<std::string> sw, sb, cw, cb;
        for (int i = 0; i < L; ++i) {
            const std::string p = "residual_layers." + std::to_string(i) + ".";
            dilated.push_back(ws.pack_conv(sd, p + "dilated_conv.weight", p + "dilated_conv.bias", 1, 3));
            out_layer.push_back(ws.pack_conv(sd, p + "output_projection.weight", p + "output_projection.bias", 1, 1));
            sw.push_back(p + "diffusion_projection.weight");
            sb.push_back(p + "diffusion_projection.bias");
            cw.push_back(p + "conditioner_projection.weight");
            cb.push_back(p + "conditioner_projection.bias");
        }
        step_all = ws.pack_concat(sd, sw, sb);
        cond_all = ws.pack_concat(sd, cw, cb);
        MAA_CHECK(step_all.N == L * cfg.residual_channels && cond_all.N == L * 2 * cfg.residual_channels, "DiffNet packing");
        skip_proj = ws.pack_conv(sd, "skip_projection.weight", "skip_projection.bias", 1, 1);
        out_proj = ws.pack_conv(sd, "output_projection.weight", "output_projection.bias", 1, 1);
    }

    // conditioner projections of every layer: cond [B, H, T] (reference layout) -> cache [B*T, L*2C]
    void set_cond(Ctx& ctx, const float* cond, int B, int T) {
        const size_t rows = (size_t)B * T;
        float* cache = static_cast<float*>(cond_cache.get(rows * cond_all.Npad * sizeof(float), ctx.stream));
        run_sized(ctx, [&] {
            float* cl = ctx.ws.alloc_f(rows * cfg.hidden_size);
            launch_nchw_to_nhwc(ctx, cond, B, cfg.hidden_size, T, cl);
            linear_into(ctx, cl, cfg.hidden_size, (long long)rows, cfg.hidden_size, cond_all, nullptr, 0, cache, cond_all.Npad);
        });
        cond_src = cond;
        cond_B = B;
        cond_T = T;
    }

    // spec [B, 1, M, T], t [B] (float), conditioning set by set_cond -> eps [B, 1, M, T]
    void forward(Ctx& ctx, const float* spec, const float* t, int B, int T, float* out) {
        MAA_CHECK(ctx.ws.dry || (cond_B == B && cond_T == T), "DiffNet: set the conditioning for this (B, T) first");
        const int C = cfg.residual_channels, L = cfg.residual_layers, M = cfg.in_dims;
        const long long rows = (long long)B * T;
        const float* cache = static_cast<const float*>(cond_cache.p);
        // x = relu(input_projection(spec))
        float* sp = ctx.ws.alloc_f((size_t)rows * M);
        launch_nchw_to_nhwc(ctx, spec, B, M, T, sp);
        float* x = ctx.ws.alloc_f((size_t)rows * C);
        {
            T4 a, o;
            a.B = o.B = B;
            a.H = o.H = 1;
            a.W = o.W = T;
            a.C = M;
            o.C = C;
            a.p = sp;
            o.p = x;
            ConvOpt co;
            co.act = 2;
            conv_into(ctx, a, nullptr, in_proj, co, o);
        }
        // diffusion-step embedding -> mlp -> all layers' diffusion_projection
        float* pe = ctx.ws.alloc_f((size_t)B * C);
        launch_ds_pos_emb(ctx, t, B, C, pe);
        float* h = ctx.ws.alloc_f((size_t)B * 4 * C);
        linear_into(ctx, pe, C, B, C, mlp0, nullptr, 0, h, 4 * C);
        launch_ds_mish(ctx, h, (long long)B * 4 * C, h);
        float* d = ctx.ws.alloc_f((size_t)B * C);
        linear_into(ctx, h, 4 * C, B, 4 * C, mlp2, nullptr, 0, d, C);
        float* steps = ctx.ws.alloc_f((size_t)B * step_all.Npad);
        linear_into(ctx, d, C, B, C, step_all, nullptr, 0, steps, step_all.Npad);

        float* xin = ctx.ws.alloc_f((size_t)rows * C);
        float* y = ctx.ws.alloc_f((size_t)rows * 2 * C);
        float* z = ctx.ws.alloc_f((size_t)rows * C);
        float* skip = ctx.ws.alloc_f((size_t)rows * C);
        launch_ds_add_step(ctx, x, steps, step_all.Npad, rows, T, C, xin);
        for (int i = 0; i < L; ++i) {
            const int dil = 1 << (i % cfg.dilation_cycle_length);
            T4 a, o;
            a.B = o.B = B;
            a.H = o.H = 1;
            a.W = o.W = T;
            a.C = C;
            o.C = 2 * C;
            a.p = xin;
            o.p = y;
            // y = dilated_conv(x + step) + conditioner_projection(cond)     (net.py:71-74)
            IGemm p;
            p.a1 = xin;
            p.lda1 = C;
            p.C1 = C;
            p.Hin = p.Hout = 1;
            p.Win = p.Wout = T;
            p.KH = 1;
            p.KW = 3;
            p.dw = dil;
            p.pw = dil;
            p.b = dilated[i].w;
            p.ldb = dilated[i].ld;
            p.b_nk = dilated[i].nk;
            p.b_split = dilated[i].split;
            p.M = (int)rows;
            p.K = 3 * C;
            p.N = 2 * C;
            p.bias = dilated[i].bias;
            p.res = cache + (size_t)i * 2 * C;
            p.ldr = cond_all.Npad;
            p.c = y;
            p.ldc = 2 * C;
            launch_igemm(ctx, p);
            launch_ds_gate(ctx, y, rows, C, z);
            // y2 = output_projection(z);  x = (x + y2[:C]) / sqrt(2);  skip += y2[C:]     (:78-81)
            linear_into(ctx, z, C, rows, C, out_layer[i], nullptr, 0, y, 2 * C);
            const bool last = i + 1 == L;
            launch_ds_residual(ctx, y, rows, T, C, x, skip, i == 0, last ? nullptr : steps + (size_t)(i + 1) * C,
                               step_all.Npad, xin);
        }
        // x = relu(skip_projection(sum(skip) / sqrt(L)));  out = output_projection(x)      (net.py:125-129)
        {
            IGemm p;
            p.a1 = skip;
            p.lda1 = C;
            p.C1 = C;
            p.M = (int)rows;
            p.K = C;
            p.N = C;
            p.b = skip_proj.w;
            p.ldb = skip_proj.ld;
            p.b_nk = skip_proj.nk;
            p.b_split = skip_proj.split;
            p.bias = skip_proj.bias;
            p.alpha = 1.0f / std::sqrt((float)L);
            p.act = 2;
            p.c = z;
            p.ldc = C;
            launch_igemm(ctx, p);
        }
        float* o80 = ctx.ws.alloc_f((size_t)rows * M);
        linear_into(ctx, z, C, rows, C, out_proj, nullptr, 0, o80, M);
        launch_nhwc_to_nchw(ctx, o80, B, M, T, out, M);
    }
};

DiffNet::DiffNet(const maa_diffnet_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    impl_->cfg = cfg;
    impl_->build(sd);
}
DiffNet::~DiffNet() = default;
const maa_diffnet_config& DiffNet::config() const { return impl_->cfg; }

void DiffNet::forward(Ctx& ctx, const float* spec, const float* t, const float* cond, int B, int T, float* out) {
    Impl& m = *impl_;
    PrecisionGuard pg(ctx, m.precision);
    m.set_cond(ctx, cond, B, T);
    run_sized(ctx, [&] { m.forward(ctx, spec, t, B, T, out); });
}

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void DiffNet::plms_sample(Ctx& ctx, const maa_plms_args& a, float* d_x) {
    Impl& m = *impl_;
    MAA_CHECK(a.B > 0 && a.T > 0 && a.K_step > 0 && a.interval > 0 && a.timesteps >= a.K_step && a.h_alphas_cumprod && a.d_cond,
              "bad plms arguments");
    MAA_CHECK(a.B <= 256, "plms: at most 256 samples per call (the step-advance kernel is one workgroup)");
    PrecisionGuard pg(ctx, m.precision);
    const int B = a.B, T = a.T, M = m.cfg.in_dims;
    const long long n = (long long)B * M * T;
    m.set_cond(ctx, a.d_cond, B, T);
    // loop state: alphas_cumprod table, {t, history count, ring head}, timestep slot, eps, eps_prev / x_pred, history ring
    auto up = [](size_t k) { return (k + 63) / 64 * 64; };
    const size_t o_ac = 0, o_st = o_ac + up(a.timesteps), o_t = o_st + 64, o_e = o_t + up(B), o_e2 = o_e + up(n),
                 o_xp = o_e2 + up(n), o_h = o_xp + up(n), total = o_h + 3 * up(n);
    float* slab = static_cast<float*>(m.loop.get(total * sizeof(float), ctx.stream));
    float *ac = slab + o_ac, *t_slot = slab + o_t, *e = slab + o_e, *e2 = slab + o_e2, *xp = slab + o_xp, *hist = slab + o_h;
    int* st = reinterpret_cast<int*>(slab + o_st);
    // first t of reversed(range(0, K_step, interval))
    const int t0 = ((a.K_step - 1) / a.interval) * a.interval;
    const int nsteps = t0 / a.interval + 1;
    const int h_st[3] = {t0, 0, 0};
    MAA_HIP(hipMemcpyAsync(ac, a.h_alphas_cumprod, (size_t)a.timesteps * 4, hipMemcpyHostToDevice, ctx.stream));
    MAA_HIP(hipMemcpyAsync(st, h_st, sizeof(h_st), hipMemcpyHostToDevice, ctx.stream));
    const long long hstride = (long long)up(n);
    (void)hstride;
    auto denoise = [&](const float* x, float* out) { run_sized(ctx, [&] { m.forward(ctx, x, t_slot, B, T, out); }); };

    // ---- first step (:184-187): predictor with e, second evaluation at max(t - interval, 0), corrector with the mean
    launch_ds_fill(ctx, t_slot, B, (float)t0);
    denoise(d_x, e);
    launch_ds_plms(ctx, d_x, e, nullptr, hist, n, ac, a.interval, st, 1, xp);
    launch_ds_fill(ctx, t_slot, B, (float)std::max(t0 - a.interval, 0));
    denoise(xp, e2);
    launch_ds_plms(ctx, d_x, e, e2, hist, n, ac, a.interval, st, 2, nullptr);
    launch_ds_plms_advance(ctx, st, a.interval, t_slot, B);

    // ---- remaining steps: identical launches on identical addresses -> one hipGraph, captured for this call and replayed
    StepGraph sg;
    run_steps(ctx, sg, nsteps - 1, a.use_graph != 0, true, [] { return std::vector<unsigned long long>(); }, [&]() {
        ctx.ws.reset();
        m.forward(ctx, d_x, t_slot, B, T, e);          // (workspace already sized by the eager evaluations above)
        launch_ds_plms(ctx, d_x, e, nullptr, hist, n, ac, a.interval, st, 0, nullptr);
        launch_ds_plms_advance(ctx, st, a.interval, t_slot, B);
    });
    MAA_HIP(hipStreamSynchronize(ctx.stream));      // (sg is dropped after it)
}

// The ancestral chain (shallow_diffusion_tts.py:269-271 / :320-321 over p_sample, :159-166).  Loop state in Impl::loop, which the
// PLMS loop also uses (every call writes all of its own): the coefficient table [timesteps][5], {t, steps done, -}, the timestep
// slot, eps.  The step reads t from the state and takes its noise at draw start - t of the caller's buffer, so the captured step
// carries no host data; ds_plms_advance_kernel with interval 1 moves t and writes the next evaluation's timestep slot.
void DiffNet::ddpm_sample(Ctx& ctx, const maa_ds_ddpm_args& a, float* d_x) {
    Impl& m = *impl_;
    const int B = a.B, T = a.T, M = m.cfg.in_dims;
    MAA_CHECK(B > 0 && T > 0 && a.timesteps > 0, "ds_ddpm_sample: empty problem");
    MAA_CHECK(a.n >= 1, "ds_ddpm_sample: the number of steps n must be at least 1");
    MAA_CHECK(a.start >= 0 && a.start < a.timesteps, "ds_ddpm_sample: start lies outside the schedule (0 <= start < timesteps)");
    MAA_CHECK(a.start - a.n + 1 >= 0, "ds_ddpm_sample: the steps run past t = 0 (start - n + 1 < 0)");
    MAA_CHECK(a.h_sqrt_recip_ac && a.h_sqrt_recipm1_ac && a.h_coef1 && a.h_coef2 && a.h_sigma,
              "ds_ddpm_sample: the posterior tables are missing");
    MAA_CHECK(a.d_cond, "ds_ddpm_sample: the conditioning d_cond is missing");
    MAA_CHECK(a.d_noise, "ds_ddpm_sample: the steps' noise d_noise is missing");
    MAA_CHECK(B <= 256, "ds_ddpm_sample: at most 256 samples per call (the step-advance kernel is one workgroup)");
    MAA_CHECK(M % 4 == 0, "ds_ddpm_sample: in_dims must be a multiple of 4 (16-byte accesses)");
    MAA_CHECK(aligned16(d_x) && aligned16(a.d_noise), "ds_ddpm_sample: d_x and d_noise must be 16-byte aligned");
    PrecisionGuard pg(ctx, m.precision);
    const long long n = (long long)B * M * T;
    m.set_cond(ctx, a.d_cond, B, T);
    auto up = [](size_t k) { return (k + 63) / 64 * 64; };
    const size_t o_tab = 0, o_st = o_tab + up((size_t)5 * a.timesteps), o_t = o_st + 64, o_e = o_t + up(B), total = o_e + up(n);
    float* slab = static_cast<float*>(m.loop.get(total * sizeof(float), ctx.stream));
    float *tab = slab + o_tab, *t_slot = slab + o_t, *e = slab + o_e;
    int* st = reinterpret_cast<int*>(slab + o_st);
    const std::vector<float> h_tab = posterior_rows(a.h_sqrt_recip_ac, a.h_sqrt_recipm1_ac, a.h_coef1, a.h_coef2, a.timesteps,
                                                    [&](int t) { return a.h_sigma[t]; });      // (row 0: nonzero_mask, :165)
    const int h_st[3] = {a.start, 0, 0};
    MAA_HIP(hipMemcpyAsync(tab, h_tab.data(), h_tab.size() * sizeof(float), hipMemcpyHostToDevice, ctx.stream));
    MAA_HIP(hipMemcpyAsync(st, h_st, sizeof(h_st), hipMemcpyHostToDevice, ctx.stream));
    MAA_HIP(hipStreamSynchronize(ctx.stream));      // (the host copies above may go out of scope on an error below)
    const int clip = a.clip_denoised ? 1 : 0;
    auto update = [&]() {
        launch_ds_ddpm_step(ctx, d_x, e, a.d_noise, n, tab, a.timesteps, st, a.start, a.n, clip);
        launch_ds_plms_advance(ctx, st, 1, t_slot, B);
    };
    // ---- first step: eager, sizes the workspace
    launch_ds_fill(ctx, t_slot, B, (float)a.start);
    run_sized(ctx, [&] { m.forward(ctx, d_x, t_slot, B, T, e); });
    update();
    // ---- remaining steps: one step, captured for this call, replayed
    StepGraph sg;
    run_steps(ctx, sg, a.n - 1, a.use_graph != 0, true, [] { return std::vector<unsigned long long>(); }, [&]() {
        ctx.ws.reset();
        m.forward(ctx, d_x, t_slot, B, T, e);
        update();
    });
    MAA_HIP(hipStreamSynchronize(ctx.stream));      // (sg is dropped after it)
}

void ds_ddpm_update(Ctx& ctx, const float* d_eps, const float* d_t, const float* d_noise, const float* h_sqrt_recip_ac,
                    const float* h_sqrt_recipm1_ac, const float* h_coef1, const float* h_coef2, const float* h_sigma, int timesteps,
                    int B, int M, int T, bool clip, float* d_x) {
    MAA_CHECK(B > 0 && M > 0 && T > 0 && timesteps > 0, "ds_ddpm_update: empty shape or table");
    MAA_CHECK(M % 4 == 0, "ds_ddpm_update: M must be a multiple of 4 (16-byte accesses)");
    MAA_CHECK(aligned16(d_x) && aligned16(d_eps) && aligned16(d_noise), "ds_ddpm_update: d_x, d_eps and d_noise must be 16-byte aligned");
    FlaggedTable ft(ctx, ctx.ddpm_scratch, posterior_rows(h_sqrt_recip_ac, h_sqrt_recipm1_ac, h_coef1, h_coef2, timesteps,
                                                         [&](int t) { return h_sigma[t]; }));
    launch_ds_ddpm_update(ctx, d_x, d_eps, d_noise, B, (long long)M * T, d_t, ft.tab, timesteps, clip ? 1 : 0, ft.bad);
    ft.check("ds_ddpm_update: some t[b] lies outside [0, timesteps)");
}

}  // namespace maa
