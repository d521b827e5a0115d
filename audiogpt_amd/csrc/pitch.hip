// Row kernels of DiffSinger's PitchExtractor (mel -> f0), channels-last [B*T, C], wave64: one wave per row, four
// channels per lane per step (C = 256: the row is one float4 per lane); reductions are wave shuffles.
//
// Replaces (NeuralSeq/): modules/fastspeech/pe.py:29-30 the padding mask, :14-18,35,40 BatchNorm1d (eval) and the
// non-padding mask of Prenet, :54,68-78,109 GroupNorm + ReLU + residual of ConvStacks; utils/__init__.py:145-157
// make_positions and modules/commons/common_layers.py:141-142 the table gather, tts_modules.py:253-254 the positional add;
// tts_modules.py:240,259 the last LayerNorm and Linear(C, 2), utils/pitch_utils.py:63-76 denorm_f0.
// All of them are memory-bound; a [1500, 256] activation is 1.5 MB and stays in L2 between launches.
// The wave reductions, the launch grid and the head's LayerNorm + Linear stage are row_device.h's (with norm.hip's LayerNorm and
// fs2.hip's duration head); the frame mask, the masked affine and the positional add also serve the FastSpeech2 front end.
#include "maa_internal.h"
#include "row_device.h"

namespace maa {
namespace {

// 256 threads: sum over the block, the same value in every thread (fixed order: bit-reproducible).  The four waves' sums add as
// (r0 + r1) + (r2 + r3), not left to right as norm.hip's block_sum does: another rounding, so the two stay apart
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// mask[row] = 0 where every bin of the frame is +-0, else 1      (pe.py:29-30, :143); hidden (optional) [row] = 1 - mask[row]
__global__ __launch_bounds__(256) void pe_frame_mask_kernel(const float* __restrict__ mel, long long rows, int M,
                                                            float* __restrict__ mask, float* __restrict__ hidden) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = mel + row * M;
    unsigned any = 0u;
    for (int c = lane * 4; c < M; c += 256) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + c);
        any |= (v.x | v.y | v.z | v.w) & 0x7fffffffu;
    }
    const unsigned long long nz = __ballot(any != 0u);
    if (lane == 0) {
        mask[row] = nz ? 1.f : 0.f;
        if (hidden) hidden[row] = nz ? 0.f : 1.f;
    }
}

// out = (x * scale + shift) * mask[row]; scale == nullptr: out = x * mask[row]      (pe.py:35 / :40)
__global__ __launch_bounds__(256) void pe_affine_mask_kernel(const float* x, long long rows, int C,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ mask, float* out) {      // (out may be x)
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float m = mask[row];
    for (int c = lane * 4; c < C; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + row * C + c);
        if (scale) {
            const float4 s = *reinterpret_cast<const float4*>(scale + c);
            const float4 h = *reinterpret_cast<const float4*>(shift + c);
            v.x = v.x * s.x + h.x;
            v.y = v.y * s.y + h.y;
            v.z = v.z * s.z + h.z;
            v.w = v.w * s.w + h.w;
        }
        v.x *= m;
        v.y *= m;
        v.z *= m;
        v.w *= m;
        *reinterpret_cast<float4*>(out + row * C + c) = v;
    }
}

// GroupNorm statistics: one block per (sample, group) over all T frames -> tab[(b * C + c) * 2] = {gamma * rstd,
// beta - mean * gamma * rstd}.  Two passes (mean, then the centred squares): the second re-reads T * cpg floats from L2.
__global__ __launch_bounds__(256) void pe_gn_stats_kernel(const float* __restrict__ x, int T, int C, int groups, float eps,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ tab) {
    __shared__ float red[4];
    const int cpg = C / groups, q = cpg >> 2;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
    const float* src = x + (long long)b * T * C + g * cpg;
    const int n4 = T * q;
    const float n = (float)T * (float)cpg;
    float s = 0.f;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const int t = i / q, qq = i - t * q;
        const float4 v = *reinterpret_cast<const float4*>(src + (long long)t * C + qq * 4);
        s += (v.x + v.y) + (v.z + v.w);
    }
    const float mean = block_sum(s, red) / n;
    float sq = 0.f;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const int t = i / q, qq = i - t * q;
        const float4 v = *reinterpret_cast<const float4*>(src + (long long)t * C + qq * 4);
        const float a = v.x - mean, e = v.y - mean, c = v.z - mean, d = v.w - mean;
        sq += (a * a + e * e) + (c * c + d * d);
    }
    const float rstd = 1.f / sqrtf(block_sum(sq, red) / n + eps);
    if ((int)threadIdx.x < cpg) {
        const int cc = g * cpg + threadIdx.x;
        const float sc = gamma[cc] * rstd;
        tab[2 * ((long long)b * C + cc)] = sc;
        tab[2 * ((long long)b * C + cc) + 1] = beta[cc] - mean * sc;
    }
}

// out = res + relu(y * scale + shift), {scale, shift} of the row's sample      (pe.py:75-76, :109)
__global__ __launch_bounds__(256) void pe_gn_relu_res_kernel(const float* y, const float* __restrict__ res,
                                                             const float* __restrict__ tab, long long rows, int T, int C,
                                                             float* out) {      // (out may be y)
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* tb = tab + 2 * (row / T) * C;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(y + row * C + c);
        const float4 r = *reinterpret_cast<const float4*>(res + row * C + c);
        const float4 t0 = *reinterpret_cast<const float4*>(tb + 2 * c);          // {sc, sh, sc, sh}
        const float4 t1 = *reinterpret_cast<const float4*>(tb + 2 * c + 4);
        float4 o;
        o.x = r.x + fmaxf(v.x * t0.x + t0.y, 0.f);
        o.y = r.y + fmaxf(v.y * t0.z + t0.w, 0.f);
        o.z = r.z + fmaxf(v.z * t1.x + t1.y, 0.f);
        o.w = r.w + fmaxf(v.w * t1.z + t1.w, 0.f);
        *reinterpret_cast<float4*>(out + row * C + c) = o;
    }
}

// make_positions on channel 0: pos[b, t] = #{t' <= t : x[b, t', 0] != 0} where x[b, t, 0] != 0, else 0.  One block per sample;
// 256 frames per step: a ballot per wave, the waves' counts through LDS, the running count carried in a register.
__global__ __launch_bounds__(256) void pe_positions_kernel(const float* __restrict__ x, int T, int C, int* __restrict__ pos) {
    __shared__ int cnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* src = x + (long long)blockIdx.x * T * C;
    int* dst = pos + (long long)blockIdx.x * T;
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        const bool nz = t < T && src[(long long)t * C] != 0.f;
        const unsigned long long bal = __ballot(nz);
        const int below = __popcll(bal & ((2ull << lane) - 1ull));          // lanes 0 .. lane, this one included
        __syncthreads();
        if (lane == 0) cnt[w] = __popcll(bal);
        __syncthreads();
        int before = carry;
        for (int i = 0; i < w; ++i) before += cnt[i];
        if (t < T) dst[t] = nz ? before + below : 0;
        carry += (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
    }
}

// out = x + alpha * table[pos[row]]      (tts_modules.py:253-254; row 0 of the table is zero)
__global__ __launch_bounds__(256) void pe_pos_add_kernel(const float* __restrict__ x, const int* __restrict__ pos,
                                                         const float* __restrict__ table, float alpha, long long rows, int C,
                                                         float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* e = table + (long long)pos[row] * C;
    for (int c = lane * 4; c < C; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + row * C + c);
        const float4 p = *reinterpret_cast<const float4*>(e + c);
        v.x += alpha * p.x;
        v.y += alpha * p.y;
        v.z += alpha * p.z;
        v.w += alpha * p.w;
        *reinterpret_cast<float4*>(out + row * C + c) = v;
    }
}

// The predictor's last layer after its convolution (whose epilogue did the ReLU): LayerNorm over the row (kept in registers,
// C <= 256 * NR) and Linear(C, 2), denorm_f0 (all row_device.h) -> pitch_pred[row] = {f0 value, voicing logit}, f0[row].
template <int NR>
__global__ __launch_bounds__(256) void pe_head_kernel(const float* __restrict__ x, long long rows, int C,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ mask, int norm, float f0_mean, float f0_std,
                                                      int use_uv, float* __restrict__ pitch_pred, float* __restrict__ f0) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float d[2];
    ln_head_dots<NR, 2>(x + row * C, C, lane, gamma, beta, eps, w, bias, d);
    if (lane == 0) {
        *reinterpret_cast<float2*>(pitch_pred + row * 2) = make_float2(d[0], d[1]);
        f0[row] = pe_denorm_f0(d[0], d[1], mask[row], norm, f0_mean, f0_std, use_uv);
    }
}

}  // namespace

void launch_pe_frame_mask(const Ctx& ctx, const float* mel, long long rows, int M, float* mask, float* hidden) {
    if (ctx.ws.dry) return;
    MAA_CHECK(M % 4 == 0, "pitch extractor: n_mel_bins must be a multiple of 4");
    ProfScope prof(ctx, "pe_rows", 0.0, 4.0 * rows * (double)M);
    hipLaunchKernelGGL(pe_frame_mask_kernel, row_grid(rows), dim3(256), 0, ctx.stream, mel, rows, M, mask, hidden);
    MAA_HIP(hipGetLastError());
}

void launch_pe_affine_mask(const Ctx& ctx, const float* x, long long rows, int C, const float* scale, const float* shift,
                           const float* mask, float* out) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0, "pitch extractor: channel counts must be multiples of 4");
    ProfScope prof(ctx, "pe_rows", 0.0, 8.0 * rows * (double)C);
    hipLaunchKernelGGL(pe_affine_mask_kernel, row_grid(rows), dim3(256), 0, ctx.stream, x, rows, C, scale, shift, mask, out);
    MAA_HIP(hipGetLastError());
}

void launch_pe_gn_relu_res(Ctx& ctx, const float* y, const float* res, int B, int T, int C, int groups, const float* gamma,
                           const float* beta, float eps, float* out) {
    float* tab = ctx.ws.alloc_f((size_t)2 * B * C);
    if (ctx.ws.dry) return;
    MAA_CHECK(groups > 0 && C % groups == 0 && (C / groups) % 4 == 0 && C / groups <= 256, "pitch extractor: GroupNorm channels");
    const long long rows = (long long)B * T;
    ProfScope prof(ctx, "pe_rows", 0.0, 20.0 * rows * (double)C);
    hipLaunchKernelGGL(pe_gn_stats_kernel, dim3((unsigned)(B * groups)), dim3(256), 0, ctx.stream, y, T, C, groups, eps, gamma, beta,
                       tab);
    hipLaunchKernelGGL(pe_gn_relu_res_kernel, row_grid(rows), dim3(256), 0, ctx.stream, y, res, tab, rows, T, C, out);
    MAA_HIP(hipGetLastError());
}

void launch_pe_pos_add(Ctx& ctx, const float* x, int B, int T, int C, const float* table, float alpha, float* out, int* pos_out) {
    const long long rows = (long long)B * T;
    int* pos = pos_out ? pos_out : reinterpret_cast<int*>(ctx.ws.alloc_f((size_t)rows));
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0, "pitch extractor: channel counts must be multiples of 4");
    ProfScope prof(ctx, "pe_rows", 0.0, 12.0 * rows * (double)C);
    hipLaunchKernelGGL(pe_positions_kernel, dim3((unsigned)B), dim3(256), 0, ctx.stream, x, T, C, pos);
    hipLaunchKernelGGL(pe_pos_add_kernel, row_grid(rows), dim3(256), 0, ctx.stream, x, pos, table, alpha, rows, C, out);
    MAA_HIP(hipGetLastError());
}

void launch_pe_head(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                    const float* w, const float* bias, const float* mask, int norm, float f0_mean, float f0_std, int use_uv,
                    float* pitch_pred, float* f0) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0 && C <= 1024, "pitch extractor: predictor width must be a multiple of 4, at most 1024");
    ProfScope prof(ctx, "pe_rows", 0.0, 4.0 * rows * (double)C);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, row_grid(rows), dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, w, bias, mask, norm, f0_mean,
                           f0_std, use_uv, pitch_pred, f0);
    };
    if (C <= 256)
        go(pe_head_kernel<1>);
    else if (C <= 512)
        go(pe_head_kernel<2>);
    else
        go(pe_head_kernel<4>);
    MAA_HIP(hipGetLastError());
}

}  // namespace maa
