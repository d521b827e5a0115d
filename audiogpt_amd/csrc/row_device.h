// Device helpers of the one-wave-per-row kernels (norm.hip, pitch.hip, fs2.hip), wave64: the wave reductions, the row
// LayerNorm held in registers, the "last LayerNorm + narrow Linear" stage of the predictor heads and denorm_f0.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace maa {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// launch grid of a 256-thread block that gives each of its four waves one row
inline dim3 row_grid(long long rows) { return dim3((unsigned)((rows + 3) / 4)); }

// LayerNorm of one row of C <= 256 * NR channels by one wave: lane `lane` holds channels (lane + 64 i) * 4 .. + 3 in v[i], zeros
// past C.  Fixed order, the same in every kernel built on it: the sum as (x + y) + (z + w) accumulated in i order (a float4 past
// C adds zeros), the centred squares over c < C only, rstd = 1 / sqrt(q / C + eps).
template <int NR>
struct LnRow {
    float4 v[NR];
    float mean, rstd;

    __device__ __forceinline__ void load(const float* __restrict__ src, int C, int lane, float eps) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int c = (lane + 64 * i) * 4;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < C) t = *reinterpret_cast<const float4*>(src + c);
            v[i] = t;
            s += (t.x + t.y) + (t.z + t.w);
        }
        mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < C) {
                const float a = v[i].x - mean, b = v[i].y - mean, d = v[i].z - mean, e = v[i].w - mean;
                q += (a * a + b * b) + (d * d + e * e);
            }
        }
        rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    }

    // the normalised channels c .. c + 3 = v[i] (c < C)
    __device__ __forceinline__ float4 norm(int i, int c, const float* __restrict__ gamma, const float* __restrict__ beta) const {
        const float4 g = *reinterpret_cast<const float4*>(gamma + c);
        const float4 bt = *reinterpret_cast<const float4*>(beta + c);
        return make_float4((v[i].x - mean) * rstd * g.x + bt.x, (v[i].y - mean) * rstd * g.y + bt.y,
                           (v[i].z - mean) * rstd * g.z + bt.z, (v[i].w - mean) * rstd * g.w + bt.w);
    }
};

// A predictor's last layer after its convolution: d[o] = LayerNorm(row) . w[o, :] + bias[o] for the NOUT rows of w [NOUT, C],
// the same values in every lane.  Each dot product adds (x + y) + (z + w) per float4, in i order.
template <int NR, int NOUT>
__device__ __forceinline__ void ln_head_dots(const float* __restrict__ src, int C, int lane, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, float eps, const float* __restrict__ w,
                                             const float* __restrict__ bias, float (&d)[NOUT]) {
    LnRow<NR> r;
    r.load(src, C, lane, eps);
    const float* wrow[NOUT];      // (the rows' starts are uniform: formed once, outside the lanes' column offsets)
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        d[o] = 0.f;
        wrow[o] = w + o * C;
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < C) {
            const float4 y = r.norm(i, c, gamma, beta);
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
                const float4 wo = *reinterpret_cast<const float4*>(wrow[o] + c);
                d[o] += (y.x * wo.x + y.y * wo.y) + (y.z * wo.z + y.w * wo.w);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) d[o] = wave_sum(d[o]) + bias[o];
}

// denorm_f0 (utils/pitch_utils.py:63-76).  norm 0: 2 ** v; 1: v * f0_std + f0_mean.  use_uv: 0 where uv (a voicing logit, or a
// caller's flag) is > 0; then 0 where the frame is padding.  Shared by the extractor's head (pitch.hip) and the cascade front
// end's pitch tail (fs2.hip).
__device__ __forceinline__ float pe_denorm_f0(float v, float uv, float live, int norm, float f0_mean, float f0_std, int use_uv) {
    float f = norm == 0 ? exp2f(v) : v * f0_std + f0_mean;
    if (use_uv && uv > 0.f) f = 0.f;
    if (live == 0.f) f = 0.f;
    return f;
}

}  // namespace maa
