// The step kernels of the five sampling loops (all HBM-bound, grid-stride, coalesced; under 0.2 % of a step).
//   Make-An-Audio (csrc/ddim.cpp):
//     CFG combine + DDIM x_{t-1} update        ldm/models/diffusion/ddim.py:199, 210-225
//     stochastic_encode (SDEdit)               ddim.py:227-241
//     PLMSSampler                              ldm/models/diffusion/plms.py:115-236
//     ancestral chain                          ddpm_audio.py:717-777, ddpm.py:214-227
//   DiffSinger (csrc/diffnet.cpp; NeuralSeq/modules/diff/shallow_diffusion_tts.py):
//     p_sample_plms                            :166-201 (get_x_pred and the 1st..4th-order pseudo linear multistep combinations)
//     p_sample                                 :134-166 (predict_start_from_noise, p_mean_variance's clamp, q_posterior's mean)
// Every formula is in torch's term order (-ffp-contract=off), divisions kept.  What two loops compute alike is one device
// helper below, so both round alike.
#include "elementwise_launch.h"

namespace maa {
namespace {

// V floats per thread (V = 4: 16-byte accesses; needs per % 4 == 0 so that a vector never straddles two samples)
template <int V>
struct FVec {
    float v[V];
};
template <int V>
__device__ __forceinline__ FVec<V> load_v(const float* p) {
    FVec<V> r;
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) r.v[k] = p[k];
    }
    return r;
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const FVec<V>& r) {
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
#pragma unroll
        for (int k = 0; k < V; ++k) p[k] = r.v[k];
}

// One step's coefficient slot, written by the prepare kernel: {a_t, a_prev, sigma, sqrt(1 - a_t), sqrt(ac_t), sqrt(1 - ac_t), log
// slot, DDIM index}.  The index comes from here and not from *step: *step is decremented by one thread of the step kernel
// while other blocks may still be starting.  kIndexed = false: the four floats of maa_ddim_update's buffer, which has no more.
struct StepCoef {
    float sigma, somat, sqrt_at, sqrt_ap, dir;
    int slot, idx;
};
template <bool kIndexed = true>
__device__ __forceinline__ StepCoef read_coef(const float* __restrict__ coef) {
    StepCoef c;
    c.idx = kIndexed ? (int)coef[7] : 0;
    const float a_t = coef[0], a_prev = coef[1];
    c.sigma = coef[2], c.somat = coef[3];
    c.slot = kIndexed ? (int)coef[6] : -1;
    c.sqrt_at = sqrtf(a_t), c.sqrt_ap = sqrtf(a_prev), c.dir = sqrtf(1.f - a_prev - c.sigma * c.sigma);
    return c;
}

// classifier-free guidance (ddim.py:199): e = eu + scale (ec - eu); ec = null: e = eu
template <int V>
__device__ __forceinline__ FVec<V> cfg_eps(const float* __restrict__ eu, const float* __restrict__ ec, float scale, long long i) {
    FVec<V> e = load_v<V>(eu + i);
    if (ec) {
        const FVec<V> c = load_v<V>(ec + i);
#pragma unroll
        for (int k = 0; k < V; ++k) e.v[k] = e.v[k] + scale * (c.v[k] - e.v[k]);
    }
    return e;
}

// get_x_prev_and_pred_x0 (ddim.py:210-225, plms.py:206-222) without its noise term: pred_x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t),
// x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) e.  The DDIM step adds sigma z temperature to that sum; PLMS has
// sigma = 0 and forms no noise term.
template <int V>
__device__ __forceinline__ void ddim_x_prev(const FVec<V>& x, const FVec<V>& e, const StepCoef& c, FVec<V>& x_prev, FVec<V>& x0) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
        x0.v[k] = (x.v[k] - c.somat * e.v[k]) / c.sqrt_at;
        x_prev.v[k] = c.sqrt_ap * x0.v[k] + c.dir * e.v[k];
    }
}

// the step's x_{t-1} / pred_x0 into the log slabs when the device table says this index is logged (ddim.py:161-163)
template <int V>
__device__ __forceinline__ void store_logged(int slot, long long n, long long i, float* __restrict__ log_x, float* __restrict__ log_x0,
                                             const FVec<V>& x_prev, const FVec<V>& x0) {
    if (slot >= 0 && log_x) {
        store_v<V>(log_x + (long long)slot * n + i, x_prev);
        store_v<V>(log_x0 + (long long)slot * n + i, x0);
    }
}

// Adams-Bashforth over this evaluation e and the history h_k = the e of k steps ago (plms.py:226-233,
// shallow_diffusion_tts.py:186-196): order 1, order 2, and order 3 for every other value.  h1 .. h3 point at this thread's
// elements; only the history the order needs is read.  h3 may be the slab this step's e is stored to afterwards.
template <int V>
__device__ __forceinline__ FVec<V> adams_bashforth(int order, const FVec<V>& e, const float* h1, const float* h2, const float* h3) {
    FVec<V> ep;
    if (order == 1) {
        const FVec<V> p1 = load_v<V>(h1);
#pragma unroll
        for (int k = 0; k < V; ++k) ep.v[k] = (3.f * e.v[k] - p1.v[k]) / 2.f;
    } else {
        const FVec<V> p1 = load_v<V>(h1), p2 = load_v<V>(h2);
        if (order == 2) {
#pragma unroll
            for (int k = 0; k < V; ++k) ep.v[k] = ((23.f * e.v[k] - 16.f * p1.v[k]) + 5.f * p2.v[k]) / 12.f;
        } else {
            const FVec<V> p3 = load_v<V>(h3);
#pragma unroll
            for (int k = 0; k < V; ++k)
                ep.v[k] = (((55.f * e.v[k] - 59.f * p1.v[k]) + 37.f * p2.v[k]) - 9.f * p3.v[k]) / 24.f;
        }
    }
    return ep;
}

// The mean of one ancestral step (ddpm.py:214-227, shallow_diffusion_tts.py:134-160), c = {sqrt_recip_ac, sqrt_recipm1_ac,
// coef1, coef2} of the timestep:
//   x_recon = c0 x - c1 e            predict_start_from_noise     (clamped to [-1, 1] when clip)
//   mean    = c2 x_recon + c3 x      q_posterior
// The noise term stays with the caller: the two families' contracts differ.
template <int V>
__device__ __forceinline__ FVec<V> posterior_mean(const FVec<V>& x, const FVec<V>& e, const float* c, bool clip, FVec<V>& x_recon) {
    FVec<V> mean;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        float r = c[0] * x.v[k] - c[1] * e.v[k];
        if (clip) r = fminf(fmaxf(r, -1.f), 1.f);
        x_recon.v[k] = r;
        mean.v[k] = c[2] * r + c[3] * x.v[k];
    }
    return mean;
}

// ---- DDIMSampler

// maa_ddim_update: one update on a plain latent.  (x and x_prev may be the same buffer -- the sampler updates the latent in place
// -- so neither is __restrict__)
__global__ void ddim_update_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float scale,
                                   const float* __restrict__ coef, long long n, float* x_prev, float* __restrict__ pred_x0) {
    const StepCoef c = read_coef<false>(coef);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const FVec<1> e = cfg_eps<1>(eu, ec, scale, i);
        FVec<1> xp, x0;
        ddim_x_prev<1>(load_v<1>(x + i), e, c, xp, x0);
        x_prev[i] = xp.v[0];
        if (pred_x0) pred_x0[i] = x0.v[0];
    }
}

// The sampling loop's form of the update (ddim.py:199, 210-225 in full): x is read from the step's UNet input (the first B
// samples of xin hold the -- possibly mask-blended -- latent, per_in elements apart), noise = sigma_t * z * temperature with the
// caller's z of this step (eta > 0), and the step's x_{t-1} / pred_x0 are copied into the log slabs when the device table
// says this index is logged (ddim.py:161-163).  Term order as the reference: (sqrt(a_prev) x0 + dir e) + noise.
__global__ void ddim_step_kernel(const float* __restrict__ xin, long long per, long long per_in, const float* __restrict__ eu,
                                 const float* __restrict__ ec, float scale, const float* __restrict__ coef, long long n,
                                 float* __restrict__ x_prev, const float* __restrict__ noise_p, float temperature, int S,
                                 float* __restrict__ log_x, float* __restrict__ log_x0, int* __restrict__ step) {
    const StepCoef c = read_coef(coef);
    if (blockIdx.x == 0 && threadIdx.x == 0) *step = c.idx - 1;
    const float* z = noise_p ? noise_p + (long long)(S - 1 - c.idx) * n : nullptr;      // visiting order: i = S - 1 - index
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const FVec<1> e = cfg_eps<1>(eu, ec, scale, i);
        const long long b = i / per;
        FVec<1> xp, x0;
        ddim_x_prev<1>(load_v<1>(xin + b * per_in + (i - b * per)), e, c, xp, x0);
        if (z) xp.v[0] = xp.v[0] + c.sigma * z[i] * temperature;
        x_prev[i] = xp.v[0];
        store_logged<1>(c.slot, n, i, log_x, log_x0, xp, x0);
    }
}

// SDEdit's forward noising, DDIMSampler.stochastic_encode (ddim.py:227-241):
//   out[b] = A[t[b]] * x0[b] + B[t[b]] * noise[b]      (extract_into_tensor gathers one row per sample; term order as torch's)
// tab = [A | B], n_tab floats each; t [B] int32 on the device.  moments != null: x0 is formed here from the VAE moments
// [B, 2C, H, W] (mean | logvar) and the posterior noise, as DiagonalGaussianDistribution.sample() followed by
// get_first_stage_encoding (ldm/latent_diffusion.py): x0 = scale_factor * (mean + exp(0.5 * clamp(logvar, -30, 20)) * n_post).
// An index outside [0, n_tab) raises *bad and writes zeros: the table is never read out of bounds.
template <int V>
__global__ void ddim_stochastic_encode_kernel(const float* __restrict__ x0, const float* __restrict__ moments, float scale_factor,
                                              const float* __restrict__ n_post, const int* __restrict__ t,
                                              const float* __restrict__ tab, int n_tab, const float* __restrict__ noise,
                                              long long per, long long n, float* __restrict__ out, int* __restrict__ bad) {
    const long long nv = n / V;
    for (long long iv = blockIdx.x * (long long)blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
        const long long i = iv * V;
        const long long b = i / per, r = i - b * per;
        const int ti = t[b];
        FVec<V> o;
        if (ti < 0 || ti >= n_tab) {
            *bad = 1;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = 0.f;
            store_v<V>(out + i, o);
            continue;
        }
        const float ca = tab[ti], cb = tab[n_tab + ti];
        FVec<V> x;
        if (moments) {
            const FVec<V> mean = load_v<V>(moments + b * 2 * per + r), lv = load_v<V>(moments + b * 2 * per + per + r);
            const FVec<V> z = load_v<V>(n_post + i);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float sd = expf(0.5f * fminf(fmaxf(lv.v[k], -30.f), 20.f));
                x.v[k] = scale_factor * (mean.v[k] + sd * z.v[k]);
            }
        } else {
            x = load_v<V>(x0 + i);
        }
        const FVec<V> z = load_v<V>(noise + i);
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = ca * x.v[k] + cb * z.v[k];
        store_v<V>(out + i, o);
    }
}

// UNet input and scalars of one DDIM step, with nothing from the host: idx = *step selects the row of the device
// tables; xin[b'] = cat(x[b' % B], concat[b' % B]) for b' < nB (nB = 2B duplicates the latents for CFG in the order
// [uncond ; cond], ddim.py:177-179; concat is the inpaint model's conditioning, ddpm.py:1404-1406).
// mask != null (ddim.py:147-150): the latent is first blended with the noised original,
//   img = q_sample(x0, t) * mask + (1 - mask) * img,   q_sample = sqrt(ac_t) x0 + sqrt(1 - ac_t) z   (ddpm.py:272-275)
// with the caller's z of this step; the blended latent only exists inside xin (the update kernel reads it from there).
__global__ void ddim_prepare_kernel(const float* __restrict__ x, const float* __restrict__ concat, int B, int nB,
                                    long long per, long long per_c, const float* __restrict__ tab_t,
                                    const float* __restrict__ tab_coef, const int* __restrict__ step,
                                    float* __restrict__ xin, float* __restrict__ cur_t, float* __restrict__ cur_coef,
                                    const float* __restrict__ mask, const float* __restrict__ x0, const float* __restrict__ noise_q,
                                    int S, const float* __restrict__ emb_tab, int emb_w, float* __restrict__ cur_emb, int n_t) {
    const int idx = *step;
    if (emb_tab)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < emb_w; i += gridDim.x * blockDim.x) cur_emb[i] = emb_tab[(long long)idx * emb_w + i];
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < n_t; k += blockDim.x) cur_t[k] = tab_t[idx];      // (n_t = nB, or one slot per crop row)
        if (threadIdx.x < 8) cur_coef[threadIdx.x] = tab_coef[idx * 8 + threadIdx.x];
    }
    const float sq_ac = tab_coef[idx * 8 + 4], sq_1mac = tab_coef[idx * 8 + 5];
    const float* z = noise_q ? noise_q + (long long)(S - 1 - idx) * B * per : nullptr;
    const long long per_in = per + per_c, n = (long long)nB * per_in;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int bb = (int)(i / per_in);
        const long long r = i - bb * per_in;
        const int b = bb % B;
        float v;
        if (r < per) {
            v = x[b * per + r];
            if (mask) {
                const long long e = b * per + r;
                const float orig = sq_ac * x0[e] + sq_1mac * z[e];
                v = orig * mask[e] + (1.f - mask[e]) * v;
            }
        } else {
            v = concat[b * per_c + (r - per)];
        }
        xin[i] = v;
    }
}

// ---- PLMSSampler (plms.py:115-236): the DDIM update with sigma = 0 applied to a combination e' of the step's eps.
// The loop's state is the DDIM loop's (csrc/ddim.cpp) plus a ring of three [B, per] slabs holding the last first evaluations
// e_t: step i (i = S - 1 - idx, idx the DDIM index in the coefficient slot) writes its e_t to slot i % 3 and reads h_k, the
// e_t of step i - k, from slot (i - k) % 3.  Everything follows from the device index, so steps 1 .. S-1 launch the same
// kernels on the same addresses.  V = 4 needs per % 4 == 0 and per_in % 4 == 0.

// Steps i >= 1 (plms.py:226-233): Adams-Bashforth of order min(i, 3) + 1 over e_t and the ring.  x is the (mask-blended)
// latent in the step's UNet input, as ddim_step_kernel reads it.  h3 and this step's e_t share slot i % 3: each thread reads
// its h3 element before it writes e_t there, so `ring` is not __restrict__.
template <int V>
__global__ void ldm_plms_step_kernel(const float* __restrict__ xin, long long per, long long per_in, const float* __restrict__ eu,
                                     const float* __restrict__ ec, float scale, const float* __restrict__ coef, long long n,
                                     float* __restrict__ x_prev, float* ring, int S, float* __restrict__ log_x,
                                     float* __restrict__ log_x0, int* __restrict__ step) {
    const StepCoef c = read_coef(coef);
    if (blockIdx.x == 0 && threadIdx.x == 0) *step = c.idx - 1;
    const int i_step = S - 1 - c.idx;
    const int order = i_step < 3 ? i_step : 3;
    float* e_slot = ring + (long long)(i_step % 3) * n;
    const float* h1 = ring + (long long)((i_step + 2) % 3) * n;
    const float* h2 = ring + (long long)((i_step + 1) % 3) * n;
    const float* h3 = e_slot;
    const long long nv = n / V;
    for (long long iv = blockIdx.x * (long long)blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
        const long long i = iv * V;
        const long long b = i / per;
        const FVec<V> e = cfg_eps<V>(eu, ec, scale, i);
        const FVec<V> x = load_v<V>(xin + b * per_in + (i - b * per));
        FVec<V> ep;
        if (order >= 1)
            ep = adams_bashforth<V>(order, e, h1 + i, h2 + i, h3 + i);
        else
            ep = e;          // (step 0 runs the Euler pair below; never reached from the loop)
        store_v<V>(e_slot + i, e);
        FVec<V> xp, x0;
        ddim_x_prev<V>(x, ep, c, xp, x0);
        store_v<V>(x_prev + i, xp);
        store_logged<V>(c.slot, n, i, log_x, log_x0, xp, x0);
    }
}

// Step 0, first half (plms.py:223-225): after the first evaluation, e_t -> ring slot 0, the blended x (first B samples of xin)
// -> x_save, x_mid = update(e_t) -> the latent channels of xin for all nB rows (the CFG duplicate too; concat channels stay),
// and the step's timestep / embedding slots move to t_next = tab_t[max(idx - 1, 0)] (plms.py:146: time_range[min(i + 1,
// len - 1)]) for the second evaluation.  Each thread reads the xin elements it then writes; no other thread reads them.
template <int V>
__global__ void ldm_plms_euler_mid_kernel(float* __restrict__ xin, long long per, long long per_in, int B, int nB,
                                          const float* __restrict__ eu, const float* __restrict__ ec, float scale,
                                          const float* __restrict__ coef, long long n, float* __restrict__ x_save,
                                          float* __restrict__ e_keep, const float* __restrict__ tab_t, float* __restrict__ cur_t,
                                          const float* __restrict__ emb_tab, int emb_w, float* __restrict__ cur_emb, int n_t) {
    const StepCoef c = read_coef(coef);
    const int idx_next = c.idx > 0 ? c.idx - 1 : 0;
    if (blockIdx.x == 0)      // (n_t = nB, or nB * L rows when the step evaluates the model on crops)
        for (int k = threadIdx.x; k < n_t; k += blockDim.x) cur_t[k] = tab_t[idx_next];
    if (emb_tab)
        for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < emb_w; k += gridDim.x * blockDim.x)
            cur_emb[k] = emb_tab[(long long)idx_next * emb_w + k];
    const long long nv = n / V;
    for (long long iv = blockIdx.x * (long long)blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
        const long long i = iv * V;
        const long long b = i / per, r = i - b * per;
        const FVec<V> e = cfg_eps<V>(eu, ec, scale, i);
        store_v<V>(e_keep + i, e);
        const FVec<V> x = load_v<V>(xin + b * per_in + r);
        store_v<V>(x_save + i, x);
        FVec<V> xm, x0;
        ddim_x_prev<V>(x, e, c, xm, x0);
        store_v<V>(xin + b * per_in + r, xm);
        if (nB > B) store_v<V>(xin + (b + B) * per_in + r, xm);
    }
}

// Step 0, second half (plms.py:226, 235): e' = (e_t + e_next) / 2 with e_next the second evaluation (CFG-combined), the update
// from the saved x into x (in place: each thread reads the element it writes), the logs, and the next DDIM index.
template <int V>
__global__ void ldm_plms_euler_final_kernel(const float* __restrict__ eu, const float* __restrict__ ec, float scale,
                                            const float* __restrict__ coef, long long n, float* x, const float* __restrict__ e_keep,
                                            float* __restrict__ log_x, float* __restrict__ log_x0, int* __restrict__ step) {
    const StepCoef c = read_coef(coef);
    if (blockIdx.x == 0 && threadIdx.x == 0) *step = c.idx - 1;
    const long long nv = n / V;
    for (long long iv = blockIdx.x * (long long)blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
        const long long i = iv * V;
        const FVec<V> en = cfg_eps<V>(eu, ec, scale, i);
        const FVec<V> et = load_v<V>(e_keep + i);
        const FVec<V> xv = load_v<V>(x + i);
        FVec<V> ep;
#pragma unroll
        for (int k = 0; k < V; ++k) ep.v[k] = (et.v[k] + en.v[k]) / 2.f;
        FVec<V> xp, x0;
        ddim_x_prev<V>(xv, ep, c, xp, x0);
        store_v<V>(x + i, xp);
        store_logged<V>(c.slot, n, i, log_x, log_x0, xp, x0);
    }
}

// ---- LatentDiffusion_audio's ancestral chain (ddpm_audio.py:717-777, ddpm.py:214-227): one DDPM step over the latent.
//   x' = posterior_mean + sd[t] (z temperature)      sd = exp(0.5 logvar_clipped[t]), 0 at t = 0 (no noise there)
// c = {the four of posterior_mean, sd, temperature}.
template <int V>
__device__ __forceinline__ void ddpm_update(const FVec<V>& x, const FVec<V>& e, const float* __restrict__ z, const float* c, bool clip,
                                            FVec<V>& xp, FVec<V>& xr) {
    xp = posterior_mean<V>(x, e, c, clip, xr);
    if (c[4] != 0.f) {      // (t = 0: the reference multiplies its draw by zero; it is not read here)
        const FVec<V> zv = load_v<V>(z);
#pragma unroll
        for (int k = 0; k < V; ++k) xp.v[k] = xp.v[k] + c[4] * (zv.v[k] * c[5]);
    }
}

// The device loop's step (csrc/ddim.cpp ddpm_sample): idx = the DDPM timestep in the step's coefficient slot (written by the
// prepare kernel), tab [T][DDPM_TAB_W] = {the six of ddpm_update, sqrt_ac, sqrt_1mac, log slot} per timestep, v = start - idx the
// visiting order that indexes the two noises.  x is read from the step's UNet input as ddim_step_kernel reads it.  The mask
// blend comes AFTER the step with the step's own t (ddpm_audio.py:873-875; DDIM blends before): x' = q_sample(x0, t) mask +
// (1 - mask) x'.  A logged step copies x' after the blend and x_recon after the clamp.  V = 4 needs per % 4 == per_in % 4 == 0.
template <int V>
__global__ void ddpm_step_kernel(const float* __restrict__ xin, long long per, long long per_in, const float* __restrict__ eu,
                                 const float* __restrict__ ec, float scale, const float* __restrict__ coef,
                                 const float* __restrict__ tab, long long n, float* __restrict__ x_prev,
                                 const float* __restrict__ noise_p, int start, int clip, const float* __restrict__ mask,
                                 const float* __restrict__ x0, const float* __restrict__ noise_q, float* __restrict__ log_x,
                                 float* __restrict__ log_x0, int* __restrict__ step) {
    const int idx = (int)coef[7];
    if (blockIdx.x == 0 && threadIdx.x == 0) *step = idx - 1;
    float c[DDPM_TAB_W];
#pragma unroll
    for (int k = 0; k < DDPM_TAB_W; ++k) c[k] = tab[(long long)idx * DDPM_TAB_W + k];
    const int slot = (int)c[8];
    const long long v = start - idx;
    const float* zp = noise_p + v * n;
    const float* zq = noise_q ? noise_q + v * n : nullptr;
    const long long nv = n / V;
    for (long long iv = blockIdx.x * (long long)blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
        const long long i = iv * V;
        const long long b = i / per;
        const FVec<V> e = cfg_eps<V>(eu, ec, scale, i);
        const FVec<V> x = load_v<V>(xin + b * per_in + (i - b * per));
        FVec<V> xp, xr;
        ddpm_update<V>(x, e, zp + i, c, clip != 0, xp, xr);
        if (mask) {
            const FVec<V> m = load_v<V>(mask + i), o = load_v<V>(x0 + i), z = load_v<V>(zq + i);
#pragma unroll
            for (int k = 0; k < V; ++k) xp.v[k] = (c[6] * o.v[k] + c[7] * z.v[k]) * m.v[k] + (1.f - m.v[k]) * xp.v[k];
        }
        store_v<V>(x_prev + i, xp);
        store_logged<V>(slot, n, i, log_x, log_x0, xp, xr);
    }
}

// One step outside the loop (p_sample, ddpm_audio.py:748-777): the timestep is t[b] per sample, tab [n_tab][5] = the first five
// of ddpm_update.  An index outside [0, n_tab) raises *bad and writes zeros, as ddim_stochastic_encode_kernel.  x_prev / x_recon
// may not alias x.
template <int V>
__global__ void ddpm_update_kernel(const float* __restrict__ x, const float* __restrict__ eps, const int* __restrict__ t,
                                   const float* __restrict__ tab, int n_tab, const float* __restrict__ noise, float temperature,
                                   int clip, long long per, long long n, float* __restrict__ x_prev, float* __restrict__ x_recon,
                                   int* __restrict__ bad) {
    const long long nv = n / V;
    for (long long iv = blockIdx.x * (long long)blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
        const long long i = iv * V;
        const int ti = t[i / per];
        FVec<V> xp, xr;
        if (ti < 0 || ti >= n_tab) {
            *bad = 1;
#pragma unroll
            for (int k = 0; k < V; ++k) xp.v[k] = xr.v[k] = 0.f;
        } else {
            float c[6];
#pragma unroll
            for (int k = 0; k < 5; ++k) c[k] = tab[(long long)ti * 5 + k];
            c[5] = temperature;
            ddpm_update<V>(load_v<V>(x + i), load_v<V>(eps + i), noise + i, c, clip != 0, xp, xr);
        }
        store_v<V>(x_prev + i, xp);
        store_v<V>(x_recon + i, xr);
    }
}

// ---- DiffSinger, channels-last [B, T, C]

// One PLMS step (shallow_diffusion_tts.py:166-201).  st = {t index (counts down by `interval`), history count}.
// mode 0: e' = adams_bashforth(history count); x = get_x_pred(x, e', t); history <- e; t -= interval
// mode 1: x_out = get_x_pred(x, e, t)                       (the predictor of the very first step)
// mode 2: e' = (e + e_prev) / 2; x = get_x_pred(x, e', t); history <- e; t -= interval     (its corrector)
// hist: ring of 3 buffers [3][n]; slot of h_k = (head - k) mod 3, head = st[2].
__global__ void ds_plms_kernel(float* x, const float* __restrict__ e, const float* __restrict__ e_prev, float* hist,
                               long long n, const float* __restrict__ ac, int interval, int* __restrict__ st, int mode,
                               float* x_out) {
    const int t = st[0], cnt = st[1], head = st[2];
    const float a_t = ac[t];
    const float a_prev = t < interval ? 1.0f : ac[max(t - interval, 0)];
    const float a_t_sq = sqrtf(a_t), a_prev_sq = sqrtf(a_prev);
    const float c1 = 1.0f / (a_t_sq * (a_t_sq + a_prev_sq));
    const float c2 = 1.0f / (a_t_sq * (sqrtf((1.0f - a_prev) * a_t) + sqrtf((1.0f - a_t) * a_prev)));
    const float da = a_prev - a_t;
    const float* h1 = hist + (long long)((head + 3) % 3) * n;
    const float* h2 = hist + (long long)((head + 2) % 3) * n;
    const float* h3 = hist + (long long)((head + 1) % 3) * n;
    float* hnew = hist + (long long)((head + 1) % 3) * n;        // overwrites h3, which is read first per element
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const FVec<1> ev = load_v<1>(e + i);
        float ep;
        if (mode == 1)
            ep = ev.v[0];
        else if (mode == 2)
            ep = (ev.v[0] + e_prev[i]) / 2.0f;
        else
            ep = adams_bashforth<1>(cnt, ev, h1 + i, h2 + i, h3 + i).v[0];
        const float xv = x[i];
        const float xn = xv + da * (c1 * xv - c2 * ep);
        if (mode == 1) {
            x_out[i] = xn;
        } else {
            x[i] = xn;
            hnew[i] = ev.v[0];
        }
    }
}

// advances the loop state after a step (its own launch: every block of ds_plms_kernel reads the state) and writes the
// timestep slot of the next denoiser evaluation
__global__ void ds_plms_advance_kernel(int* st, int interval, float* __restrict__ t_slot, int B) {
    __shared__ int tn;
    if (threadIdx.x == 0) {
        tn = st[0] - interval;
        st[0] = tn;
        st[1] = st[1] + 1;
        st[2] = (st[2] + 1) % 3;
    }
    __syncthreads();
    if ((int)threadIdx.x < B) t_slot[threadIdx.x] = (float)max(tn, 0);
}

// One ancestral step of four elements in place (shallow_diffusion_tts.py:134-166: posterior_mean, then p_sample's `mean +
// nonzero_mask * (0.5 * logvar).exp() * noise`), in torch's term order.  r = one row of the table: {the four of posterior_mean,
// sigma}, sigma = 0 in row 0 (the nonzero_mask); the draw is always read.  Shared by the loop's kernel and the single-step
// kernel: both round alike.
__device__ __forceinline__ void ds_ddpm_four(float* x, const float* __restrict__ e, const float* __restrict__ z, const float* r,
                                             int clip) {
    FVec<4> xr;
    FVec<4> xp = posterior_mean<4>(load_v<4>(x), load_v<4>(e), r, clip != 0, xr);
    const FVec<4> zv = load_v<4>(z);
#pragma unroll
    for (int k = 0; k < 4; ++k) xp.v[k] = xp.v[k] + r[4] * zv.v[k];
    store_v<4>(x, xp);
}

// The loop's step: t = st[0] (device state), the step's noise is draw k = start - t of the call's buffer [n_steps][n], so a
// captured launch takes no host data.  n4 = n / 4 (n = B * M * T, M % 4 == 0).  A state outside the call's range writes nothing.
__global__ void ds_ddpm_step_kernel(float* x, const float* __restrict__ e, const float* __restrict__ noise, long long n4,
                                    const float* __restrict__ tab, int timesteps, const int* __restrict__ st, int start,
                                    int n_steps, int clip) {
    const int t = st[0], k = start - t;
    if (t < 0 || t >= timesteps || k < 0 || k >= n_steps) return;
    float r[5];
    for (int j = 0; j < 5; ++j) r[j] = tab[(long long)t * 5 + j];
    const float* z = noise + (long long)k * n4 * 4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
        ds_ddpm_four(x + 4 * i, e + 4 * i, z + 4 * i, r, clip);
}

// p_sample's arithmetic for one step with a timestep per sample: t [B] (the integer step as float, as the denoiser takes it),
// per4 = M * T / 4 vectors per sample.  A t[b] outside the table leaves its sample unchanged and raises *bad.
__global__ void ds_ddpm_update_kernel(float* x, const float* __restrict__ e, const float* __restrict__ noise, int B,
                                      long long per4, const float* __restrict__ t, const float* __restrict__ tab,
                                      int timesteps, int clip, int* __restrict__ bad) {
    const long long n4 = (long long)B * per4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per4);
        const float tf = t[b];
        const int tb = (int)tf;
        if (!(tf >= 0.0f) || tb >= timesteps) {
            *bad = 1;
            continue;
        }
        float r[5];
        for (int j = 0; j < 5; ++j) r[j] = tab[(long long)tb * 5 + j];
        ds_ddpm_four(x + 4 * i, e + 4 * i, noise + 4 * i, r, clip);
    }
}

bool al16(const void* p) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

// kern<4> over n / 4 vectors when vec, else kern<1> over n elements
#define MAA_LAUNCH_V(vec, kern, n, ...)                                                      \
    if (vec) {                                                                               \
        MAA_LAUNCH1(kern<4>, (n) / 4, __VA_ARGS__);                                          \
    } else {                                                                                 \
        MAA_LAUNCH1(kern<1>, n, __VA_ARGS__);                                                \
    }

void launch_ddim_update(const Ctx& ctx, const float* x, const float* eps_u, const float* eps_c, float scale,
                        const float* coef, long long n, float* x_prev, float* pred_x0) {
    MAA_LAUNCH1(ddim_update_kernel, n, x, eps_u, eps_c, scale, coef, n, x_prev, pred_x0);
}
void launch_ddim_prepare(const Ctx& ctx, const float* x, const float* concat, int B, int nB, long long per,
                         long long per_c, const float* tab_t, const float* tab_coef, const int* step, float* xin,
                         float* cur_t, float* cur_coef, const float* mask, const float* x0, const float* noise_q, int S,
                         const float* emb_tab, int emb_w, float* cur_emb, int n_t) {
    MAA_CHECK(nB <= 256, "ddim: at most 256 UNet rows per step");
    MAA_LAUNCH1(ddim_prepare_kernel, (long long)nB * (per + per_c), x, concat, B, nB, per, per_c, tab_t, tab_coef, step,
                xin, cur_t, cur_coef, mask, x0, noise_q, S, emb_tab, emb_w, cur_emb, n_t > 0 ? n_t : nB);
}
void launch_ddim_step(const Ctx& ctx, const float* xin, long long per, long long per_in, const float* eps_u, const float* eps_c,
                      float scale, const float* coef, long long n, float* x_prev, const float* noise_p, float temperature, int S,
                      float* log_x, float* log_x0, int* step) {
    MAA_LAUNCH1(ddim_step_kernel, n, xin, per, per_in, eps_u, eps_c, scale, coef, n, x_prev, noise_p, temperature, S, log_x, log_x0,
                step);
}
void launch_ddim_stochastic_encode(const Ctx& ctx, const float* x0, const float* moments, float scale_factor, const float* n_post,
                                   const int* t, const float* tab, int n_tab, const float* noise, int B, long long per, float* out,
                                   int* bad) {
    MAA_CHECK(B > 0 && per > 0 && n_tab > 0, "stochastic_encode: empty problem");
    MAA_CHECK((moments != nullptr) == (n_post != nullptr) && (moments != nullptr) != (x0 != nullptr),
              "stochastic_encode: give x0, or the moments and their posterior noise");
    const long long n = (long long)B * per;
    const bool vec = per % 4 == 0 && al16(x0) && al16(moments) && al16(n_post) && al16(noise) && al16(out);
    MAA_LAUNCH_V(vec, ddim_stochastic_encode_kernel, n, x0, moments, scale_factor, n_post, t, tab, n_tab, noise, per, n, out, bad);
}

void launch_ldm_plms_step(const Ctx& ctx, const float* xin, long long per, long long per_in, const float* eps_u, const float* eps_c,
                          float scale, const float* coef, long long n, float* x_prev, float* ring, int S, float* log_x, float* log_x0,
                          int* step) {
    MAA_CHECK(per > 0 && n % per == 0, "plms: empty problem");
    const bool vec = per % 4 == 0 && per_in % 4 == 0 && al16(xin) && al16(eps_u) && al16(eps_c) && al16(x_prev) && al16(ring) &&
                     al16(log_x) && al16(log_x0);
    MAA_LAUNCH_V(vec, ldm_plms_step_kernel, n, xin, per, per_in, eps_u, eps_c, scale, coef, n, x_prev, ring, S, log_x, log_x0, step);
}
void launch_ldm_plms_euler_mid(const Ctx& ctx, float* xin, long long per, long long per_in, int B, int nB, const float* eps_u,
                               const float* eps_c, float scale, const float* coef, float* x_save, float* e_keep, const float* tab_t,
                               float* cur_t, const float* emb_tab, int emb_w, float* cur_emb, int n_t) {
    MAA_CHECK(per > 0 && B > 0 && (nB == B || nB == 2 * B) && nB <= 256, "plms: bad step shape");
    if (n_t <= 0) n_t = nB;
    const long long n = (long long)B * per;
    const bool vec = per % 4 == 0 && per_in % 4 == 0 && al16(xin) && al16(eps_u) && al16(eps_c) && al16(x_save) && al16(e_keep);
    MAA_LAUNCH_V(vec, ldm_plms_euler_mid_kernel, n, xin, per, per_in, B, nB, eps_u, eps_c, scale, coef, n, x_save, e_keep, tab_t,
                 cur_t, emb_tab, emb_w, cur_emb, n_t);
}
void launch_ldm_plms_euler_final(const Ctx& ctx, const float* eps_u, const float* eps_c, float scale, const float* coef, long long n,
                                 float* x, const float* e_keep, float* log_x, float* log_x0, int* step) {
    MAA_CHECK(n > 0, "plms: empty problem");
    const bool vec = n % 4 == 0 && al16(eps_u) && al16(eps_c) && al16(x) && al16(e_keep) && al16(log_x) && al16(log_x0);
    MAA_LAUNCH_V(vec, ldm_plms_euler_final_kernel, n, eps_u, eps_c, scale, coef, n, x, e_keep, log_x, log_x0, step);
}

void launch_ddpm_step(const Ctx& ctx, const float* xin, long long per, long long per_in, const float* eps_u, const float* eps_c,
                      float scale, const float* coef, const float* tab, long long n, float* x_prev, const float* noise_p, int start,
                      bool clip, const float* mask, const float* x0, const float* noise_q, float* log_x, float* log_x0, int* step) {
    MAA_CHECK(per > 0 && n > 0 && n % per == 0 && noise_p, "ddpm: empty problem");
    MAA_CHECK(!mask || (x0 && noise_q), "ddpm: mask needs x0 and its noise");
    const bool vec = per % 4 == 0 && per_in % 4 == 0 && al16(xin) && al16(eps_u) && al16(eps_c) && al16(x_prev) && al16(noise_p) &&
                     al16(mask) && al16(x0) && al16(noise_q) && al16(log_x) && al16(log_x0);
    MAA_LAUNCH_V(vec, ddpm_step_kernel, n, xin, per, per_in, eps_u, eps_c, scale, coef, tab, n, x_prev, noise_p, start, (int)clip, mask,
                 x0, noise_q, log_x, log_x0, step);
}
void launch_ddpm_update(const Ctx& ctx, const float* x, const float* eps, const int* t, const float* tab, int n_tab, const float* noise,
                        float temperature, bool clip, int B, long long per, float* x_prev, float* x_recon, int* bad) {
    MAA_CHECK(B > 0 && per > 0 && n_tab > 0 && x && eps && t && tab && noise && x_prev && x_recon && bad, "ddpm_update: empty problem");
    const long long n = (long long)B * per;
    const bool vec = per % 4 == 0 && al16(x) && al16(eps) && al16(noise) && al16(x_prev) && al16(x_recon);
    MAA_LAUNCH_V(vec, ddpm_update_kernel, n, x, eps, t, tab, n_tab, noise, temperature, (int)clip, per, n, x_prev, x_recon, bad);
}

void launch_ds_plms(const Ctx& ctx, float* x, const float* e, const float* e_prev, float* hist, long long n,
                    const float* ac, int interval, int* st, int mode, float* x_out) {
    MAA_LAUNCH1(ds_plms_kernel, n, x, e, e_prev, hist, n, ac, interval, st, mode, x_out);
}
void launch_ds_plms_advance(const Ctx& ctx, int* st, int interval, float* t_slot, int B) {
    if (ctx.ws.dry) return;
    MAA_CHECK(B <= 256, "plms: at most 256 samples per call");
    hipLaunchKernelGGL(ds_plms_advance_kernel, dim3(1), dim3(256), 0, ctx.stream, st, interval, t_slot, B);
    MAA_HIP(hipGetLastError());
}
// n must be a multiple of 4 and x / e / noise 16-byte aligned (checked by the callers, DiffNet::ddpm_sample and ds_ddpm_update)
void launch_ds_ddpm_step(const Ctx& ctx, float* x, const float* e, const float* noise, long long n, const float* tab,
                         int timesteps, const int* st, int start, int n_steps, int clip) {
    MAA_LAUNCH1(ds_ddpm_step_kernel, n / 4, x, e, noise, n / 4, tab, timesteps, st, start, n_steps, clip);
}
void launch_ds_ddpm_update(const Ctx& ctx, float* x, const float* e, const float* noise, int B, long long per, const float* t,
                           const float* tab, int timesteps, int clip, int* bad) {
    MAA_LAUNCH1(ds_ddpm_update_kernel, B * per / 4, x, e, noise, B, per / 4, t, tab, timesteps, clip, bad);
}

}  // namespace maa
