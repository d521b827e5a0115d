// Row kernels of the Glow post-net run in reverse (GenerSpeech / PortaSpeech: mel-sized latent + conditioning -> mel), channels-last
// rows, wave64: one wave per row, four channels per lane per step, 16-byte loads and plain 16-byte vector stores.  The
// contractions between them -- start, the dilated in_layers, res_skip_layers, end, the hoisted cond_layer GEMM -- are glow.cpp's.
//
// Replaces (NeuralSeq/modules/GenerSpeech/model/): glow_modules.py:742-767 squeeze / unsqueeze (n_sqz = 2: a view of the
// channels-last layout, so only the mask and the dropped odd frame cost a pass), wavenet.py:5-11 fused_add_tanh_sigmoid_multiply
// (the add is the igemm's residual term), wavenet.py:72-78 the residual / skip bookkeeping with its masks, and per flow block in
// one launch glow_modules.py:320-332 the affine coupling inverse, :147-182 InvConvNear's 4 x 4 mix over channel groups and
// :77-91 ActNorm, with the row's share of the coupling's log-determinant.  A last kernel sums each sample's rows in a fixed
// order (no atomics).  All of them are memory-bound on a few hundred to a few thousand rows.
#include "maa_internal.h"
#include "models.h"
#include "row_device.h"

namespace maa {
namespace {

// Squeezed row t' of sample b is [in[b, 2t'], in[b, 2t' + 1]] (channel s * C + c) times mask_s[b, t'] = mask[b, 2t' + 1]; a
// frame 2 Ts (T odd) is never read.  mask == nullptr: all ones.  mask_out (optional) [B * Ts] receives mask_s.
__global__ __launch_bounds__(256) void glow_squeeze_kernel(const float* __restrict__ in, const float* __restrict__ mask, long long rows,
                                                           int T, int Ts, int C, float* __restrict__ out,
                                                           float* __restrict__ mask_out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long b = row / Ts;
    const int ts = (int)(row - b * Ts);
    const float m = mask ? mask[b * T + 2 * ts + 1] : 1.f;
    const float* src = in + (b * T + 2 * ts) * C;      // the two frames are neighbours: 2C contiguous floats
    float* dst = out + row * 2 * C;
    for (int c = lane * 4; c < 2 * C; c += 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m != 0.f) {
            v = *reinterpret_cast<const float4*>(src + c);
            v.x *= m;
            v.y *= m;
            v.z *= m;
            v.w *= m;
        }
        *reinterpret_cast<float4*>(dst + c) = v;
    }
    if (mask_out && lane == 0) mask_out[row] = m;
}

__device__ __forceinline__ float glow_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// acts = tanh(y[:, :H]) * sigmoid(y[:, H:]): the first half goes through tanh (DiffNet's gate has the halves the other way round)
__global__ __launch_bounds__(256) void glow_gate_kernel(const float* __restrict__ y, long long rows, int H, float* __restrict__ z) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = y + row * 2 * H;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 t = *reinterpret_cast<const float4*>(src + c);
        const float4 s = *reinterpret_cast<const float4*>(src + H + c);
        *reinterpret_cast<float4*>(z + row * H + c) = make_float4(tanhf(t.x) * glow_sigmoid(s.x), tanhf(t.y) * glow_sigmoid(s.y),
                                                                  tanhf(t.z) * glow_sigmoid(s.z), tanhf(t.w) * glow_sigmoid(s.w));
    }
}

// WN's bookkeeping after res_skip_layers[i] (wavenet.py:72-78).
// not last: rs [rows, 2H]; x = (x + rs[:, :H]) * mask; skip (+)= rs[:, H:]        (first: skip = )
// last:     rs [rows, H];  skip = (skip + rs) * mask                            (the WN's `output * x_mask`)
__global__ __launch_bounds__(256) void glow_wn_residual_kernel(const float* __restrict__ rs, long long rows, int H,
                                                               const float* __restrict__ mask, int first, int last,
                                                               float* __restrict__ x, float* __restrict__ skip) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float m = mask[row];
    const float* src = rs + row * (last ? H : 2 * H);
    for (int c = lane * 4; c < H; c += 256) {
        float4 s = *reinterpret_cast<const float4*>(src + (last ? 0 : H) + c);
        if (!first) {
            const float4 o = *reinterpret_cast<const float4*>(skip + row * H + c);
            s.x += o.x;
            s.y += o.y;
            s.z += o.z;
            s.w += o.w;
        }
        if (last) {
            s.x *= m;
            s.y *= m;
            s.z *= m;
            s.w *= m;
        } else {
            const float4 r = *reinterpret_cast<const float4*>(src + c);
            float4 v = *reinterpret_cast<const float4*>(x + row * H + c);
            v.x = (v.x + r.x) * m;
            v.y = (v.y + r.y) * m;
            v.z = (v.z + r.z) * m;
            v.w = (v.w + r.w) * m;
            *reinterpret_cast<float4*>(x + row * H + c) = v;
        }
        *reinterpret_cast<float4*>(skip + row * H + c) = s;
    }
}

// z[i'] = sum_i w[i' * 4 + i] * v[i], in i order
__device__ __forceinline__ void glow_mix4(const float* __restrict__ w, float v0, float v1, float v2, float v3, float (&z)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = ((w[i * 4] * v0 + w[i * 4 + 1] * v1) + w[i * 4 + 2] * v2) + w[i * 4 + 3] * v3;
}

// One flow block's tail in reverse, a row of 2C channels per wave: x [rows, 2C] is the block's input, eo [rows, 2C] = end(WN(..))
// = [m | logs].
//   coupling:  z1 = (x1 - m) * exp(-logs) * mask, x0 unchanged; logs = log(1e-6 + sigmoid(logs + 2)) under sigmoid_scale
//   InvConvNear: channel a * C + 2j + k is group i = 2a + k at position j; z[i', j] = sum_i winv[i', i] x[i, j], times mask.
//     A lane's float4 at c in the first half and its float4 at C + c hold the four groups of positions c / 2 and c / 2 + 1:
//     the mix never leaves the lane.
//   ActNorm:   (x - bias) * exp(-logs_an) * mask, einv = exp(-logs_an) from the host
// out [rows, 2C] (may be x): the next block's input (the last block's is the caller's x: unsqueeze is a view of this layout).
// rowld[row] (+)= sum_c(-logs * mask).  h_cpl / h_inv / h_act (optional, [rows, 2C]): the three flows' outputs.
// A masked row writes exact zeros and adds nothing.
__global__ __launch_bounds__(256) void glow_block_tail_kernel(const float* x, const float* __restrict__ eo,
                                                              const float* __restrict__ mask, long long rows, int C,
                                                              int sigmoid_scale, const float* __restrict__ winv,
                                                              const float* __restrict__ an_bias, const float* __restrict__ an_einv,
                                                              int first, float* out, float* __restrict__ rowld,
                                                              float* __restrict__ h_cpl, float* __restrict__ h_inv,
                                                              float* __restrict__ h_act) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float m = mask[row];
    const long long base = row * 2 * C;
    if (m == 0.f) {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = lane * 4; c < 2 * C; c += 256) {
            *reinterpret_cast<float4*>(out + base + c) = z4;
            if (h_cpl) *reinterpret_cast<float4*>(h_cpl + base + c) = z4;
            if (h_inv) *reinterpret_cast<float4*>(h_inv + base + c) = z4;
            if (h_act) *reinterpret_cast<float4*>(h_act + base + c) = z4;
        }
        if (lane == 0 && first) rowld[row] = 0.f;
        return;
    }
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = winv[i];
    float ld = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 x0 = *reinterpret_cast<const float4*>(x + base + c);
        const float4 x1 = *reinterpret_cast<const float4*>(x + base + C + c);
        const float4 mu = *reinterpret_cast<const float4*>(eo + base + c);
        float4 lg = *reinterpret_cast<const float4*>(eo + base + C + c);
        if (sigmoid_scale) {
            lg.x = logf(1e-6f + glow_sigmoid(lg.x + 2.f));
            lg.y = logf(1e-6f + glow_sigmoid(lg.y + 2.f));
            lg.z = logf(1e-6f + glow_sigmoid(lg.z + 2.f));
            lg.w = logf(1e-6f + glow_sigmoid(lg.w + 2.f));
        }
        ld -= ((lg.x + lg.y) + (lg.z + lg.w)) * m;
        const float4 z1 = make_float4((x1.x - mu.x) * expf(-lg.x) * m, (x1.y - mu.y) * expf(-lg.y) * m,
                                      (x1.z - mu.z) * expf(-lg.z) * m, (x1.w - mu.w) * expf(-lg.w) * m);
        if (h_cpl) {
            *reinterpret_cast<float4*>(h_cpl + base + c) = x0;
            *reinterpret_cast<float4*>(h_cpl + base + C + c) = z1;
        }
        float za[4], zb[4];
        glow_mix4(w, x0.x, x0.y, z1.x, z1.y, za);      // position c / 2
        glow_mix4(w, x0.z, x0.w, z1.z, z1.w, zb);      // position c / 2 + 1
        float4 lo = make_float4(za[0] * m, za[1] * m, zb[0] * m, zb[1] * m);
        float4 hi = make_float4(za[2] * m, za[3] * m, zb[2] * m, zb[3] * m);
        if (h_inv) {
            *reinterpret_cast<float4*>(h_inv + base + c) = lo;
            *reinterpret_cast<float4*>(h_inv + base + C + c) = hi;
        }
        const float4 b0 = *reinterpret_cast<const float4*>(an_bias + c);
        const float4 b1 = *reinterpret_cast<const float4*>(an_bias + C + c);
        const float4 e0 = *reinterpret_cast<const float4*>(an_einv + c);
        const float4 e1 = *reinterpret_cast<const float4*>(an_einv + C + c);
        lo = make_float4((lo.x - b0.x) * e0.x * m, (lo.y - b0.y) * e0.y * m, (lo.z - b0.z) * e0.z * m, (lo.w - b0.w) * e0.w * m);
        hi = make_float4((hi.x - b1.x) * e1.x * m, (hi.y - b1.y) * e1.y * m, (hi.z - b1.z) * e1.z * m, (hi.w - b1.w) * e1.w * m);
        if (h_act) {
            *reinterpret_cast<float4*>(h_act + base + c) = lo;
            *reinterpret_cast<float4*>(h_act + base + C + c) = hi;
        }
        *reinterpret_cast<float4*>(out + base + c) = lo;
        *reinterpret_cast<float4*>(out + base + C + c) = hi;
    }
    ld = wave_sum(ld);
    if (lane == 0) rowld[row] = first ? ld : rowld[row] + ld;
}

// logdet[b] = sum over the sample's Ts rows of rowld + per_len * x_len[b], x_len = sum of mask_s: one block per sample, thread i
// adds rows i, i + 256, .. in order, then a fixed tree over the 256 partial sums -- the same bits for the same inputs.
__global__ __launch_bounds__(256) void glow_logdet_kernel(const float* __restrict__ rowld, const float* __restrict__ mask, int Ts,
                                                          float per_len, float* __restrict__ logdet) {
    __shared__ float s_ld[256], s_len[256];
    const long long at = (long long)blockIdx.x * Ts;
    float a = 0.f, n = 0.f;
    for (int t = threadIdx.x; t < Ts; t += 256) {
        a += rowld[at + t];
        n += mask[at + t];
    }
    s_ld[threadIdx.x] = a;
    s_len[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_ld[threadIdx.x] += s_ld[threadIdx.x + o];
            s_len[threadIdx.x] += s_len[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) logdet[blockIdx.x] = s_ld[0] + per_len * s_len[0];
}

}  // namespace

void launch_glow_squeeze(const Ctx& ctx, const float* in, const float* mask, int B, int T, int C, float* out, float* mask_out) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0 && T >= 2, "Glow squeeze: channels must be a multiple of 4 and T at least 2");
    const int Ts = T / 2;
    const long long rows = (long long)B * Ts;
    ProfScope prof(ctx, "glow_rows", 0.0, 16.0 * rows * (double)C);
    hipLaunchKernelGGL(glow_squeeze_kernel, row_grid(rows), dim3(256), 0, ctx.stream, in, mask, rows, T, Ts, C, out, mask_out);
    MAA_HIP(hipGetLastError());
}

void launch_glow_gate(const Ctx& ctx, const float* y, long long rows, int H, float* z) {
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "Glow: hidden_channels must be a multiple of 4");
    ProfScope prof(ctx, "glow_rows", 0.0, 12.0 * rows * (double)H);
    hipLaunchKernelGGL(glow_gate_kernel, row_grid(rows), dim3(256), 0, ctx.stream, y, rows, H, z);
    MAA_HIP(hipGetLastError());
}

void launch_glow_wn_residual(const Ctx& ctx, const float* rs, long long rows, int H, const float* mask, bool first, bool last, float* x,
                             float* skip) {
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "Glow: hidden_channels must be a multiple of 4");
    ProfScope prof(ctx, "glow_rows", 0.0, 24.0 * rows * (double)H);
    hipLaunchKernelGGL(glow_wn_residual_kernel, row_grid(rows), dim3(256), 0, ctx.stream, rs, rows, H, mask, first ? 1 : 0, last ? 1 : 0,
                       x, skip);
    MAA_HIP(hipGetLastError());
}

void launch_glow_block_tail(const Ctx& ctx, const float* x, const float* eo, const float* mask, long long rows, int C, int sigmoid_scale,
                            const float* winv, const float* an_bias, const float* an_einv, bool first, float* out, float* rowld,
                            float* h_cpl, float* h_inv, float* h_act) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0, "Glow: in_channels must be a multiple of 4");
    ProfScope prof(ctx, "glow_rows", 0.0, (h_cpl ? 48.0 : 24.0) * rows * (double)C);
    hipLaunchKernelGGL(glow_block_tail_kernel, row_grid(rows), dim3(256), 0, ctx.stream, x, eo, mask, rows, C, sigmoid_scale, winv, an_bias,
                       an_einv, first ? 1 : 0, out, rowld, h_cpl, h_inv, h_act);
    MAA_HIP(hipGetLastError());
}

void launch_glow_logdet(const Ctx& ctx, const float* rowld, const float* mask, int B, int Ts, float per_len, float* logdet) {
    if (ctx.ws.dry) return;
    ProfScope prof(ctx, "glow_rows", 0.0, 8.0 * B * (double)Ts);
    hipLaunchKernelGGL(glow_logdet_kernel, dim3((unsigned)B), dim3(256), 0, ctx.stream, rowld, mask, Ts, per_len, logdet);
    MAA_HIP(hipGetLastError());
}

}  // namespace maa
