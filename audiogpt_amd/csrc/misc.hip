// Small elementwise / layout kernels of the hot path (all HBM-bound, grid-stride, coalesced).
//   timestep embedding [cos | sin]      ldm/modules/diffusionmodules/util.py:151-171
//   avg-pool 2x2 / nearest 2x           openaimodel.py:209-216 (resblock_updown), :116-118
//   BigVGAN Activation1d                vocoder/bigvgan/alias_free_torch/{act.py:23-27,resample.py:25-33,46-49,
//                                       filter.py:28-57,86-94}, activations.py:107-119
// (The sampling loops' step kernels are in sampler_steps.hip.)
#include "elementwise_launch.h"

#include <mutex>

#include <cstdlib>

#include <cmath>

namespace maa {
namespace {

__global__ void timestep_embedding_kernel(const float* __restrict__ t, int B, int dim, float* __restrict__ out) {
    const int half = dim / 2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * half; i += gridDim.x * blockDim.x) {
        const int b = i / half, j = i - b * half;
        // freqs = exp(-ln(10000) * j / half) in fp32, as torch.exp over an fp32 arange
        const float f = expf(-9.210340371976184f * (float)j / (float)half);
        const float a = t[b] * f;
        out[(long long)b * dim + j] = cosf(a);
        out[(long long)b * dim + half + j] = sinf(a);
    }
}

__global__ void silu_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = x[i];
        out[i] = v / (1.f + expf(-v));
    }
}

__global__ void scale_kernel(const float* __restrict__ x, long long n, float s, float* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = x[i] * s;
}

// x [B, C, HW] -> out [B, HW, C]
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, int B, int C, int HW, float* __restrict__ out) {
    const long long n = (long long)B * C * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long r = i / C;
        const int p = (int)(r % HW);
        const int b = (int)(r / HW);
        out[i] = x[((long long)b * C + c) * HW + p];
    }
}

// x [B, HW, ld_in] (first C channels) -> out [B, C, HW]
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ x, int B, int C, int HW, int ld_in,
                                    float* __restrict__ out) {
    const long long n = (long long)B * C * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(i % HW);
        const long long r = i / HW;
        const int c = (int)(r % C);
        const int b = (int)(r / C);
        out[i] = x[((long long)b * HW + p) * ld_in + c];
    }
}

// clamp((mel + 1) / 2, 0, 1): the line between decode_first_stage and the vocoder in every tool (audio-chatgpt.py:175-176,
// 254-255, 521-522), in the reference's operation order
__global__ void spec_from_mel_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = fminf(fmaxf((x[i] + 1.0f) / 2.0f, 0.0f), 1.0f);
}

// 3x3 convolution (stride 1, padding 1) to a FEW output channels (N <= 4: the UNet's 320 -> 4 output convolution,
// openaimodel.py:693-697) from split32 rows, written straight to NCHW.  The implicit-GEMM engines pad N to 32 and ran this layer
// on 49 - 98 workgroups of 90 K chunks (58 us for 0.3 GFLOP); here a wave owns four consecutive output positions, a lane eight
// channels (one 16-byte load of the hi halves and one of the lo halves per tap and position; x = hi + lo, 2^-17 relative), the
// weights sit in LDS as one float4 per (tap, channel) and are read once per four positions, the products are fp32 FMAs (more
// exact than the bf16x3 MFMA), the 16 partial sums are reduced across the wave at the end.
__global__ __launch_bounds__(256) void narrow_conv3x3_kernel(const float* __restrict__ a, int lda, int B, int H, int W, int C,
                                                            const float4* __restrict__ w4, const float* __restrict__ bias, int N,
                                                            float* __restrict__ out_nchw) {
    extern __shared__ __attribute__((aligned(16))) float4 sw[];      // [9 taps][8 k][C / 8 groups]: channel 8 g + k of tap t
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int i = tid; i < 9 * C; i += 256) sw[i] = w4[i];
    __syncthreads();
    const int HW = H * W;
    const long long M = (long long)B * HW;
    const long long m0 = ((long long)blockIdx.x * 4 + wid) * 4;
    if (m0 >= M) return;
    int py[4], px[4];
    bool live[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const long long m = m0 + p;
        live[p] = m < M;
        const int r = (int)((live[p] ? m : 0) % HW);
        py[p] = r / W;
        px[p] = r - py[p] * W;
    }
    float acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[p][n] = 0.f;
    const char* ab = reinterpret_cast<const char*>(a);
    // (measured, round 6: fetching the next tap's pieces before multiplying this one costs 70 more VGPRs and doubles the kernel's
    // time; unrolling the taps spills)
    for (int g = lane; g < C / 8; g += 64) {
        const long long goff = (long long)(g >> 2) * 128 + (g & 3) * 16;      // hi halves of channels 8 g .. 8 g + 7 inside a row
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            float x[4][8];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int iy = py[p] + dy, ix = px[p] + dx;
                const bool ok = live[p] && iy >= 0 && iy < H && ix >= 0 && ix < W;      // wave-uniform
                if (ok) {
                    const char* row = ab + ((m0 + p) + (long long)dy * W + dx) * (long long)lda * 4 + goff;
                    const uint4 hi = *reinterpret_cast<const uint4*>(row);
                    const uint4 lo = *reinterpret_cast<const uint4*>(row + 64);
                    const unsigned hw[4] = {hi.x, hi.y, hi.z, hi.w}, lw[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        x[p][2 * k] = __builtin_bit_cast(float, hw[k] << 16) + __builtin_bit_cast(float, lw[k] << 16);
                        x[p][2 * k + 1] = __builtin_bit_cast(float, hw[k] & 0xffff0000u) + __builtin_bit_cast(float, lw[k] & 0xffff0000u);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) x[p][k] = 0.f;
                }
            }
            const int G = C >> 3;
            const float4* wt = sw + (t * 8) * G + g;      // [tap][k][g]: the lanes of a wave read consecutive float4 (no bank conflicts)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 wv = wt[k * G];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    acc[p][0] = fmaf(x[p][k], wv.x, acc[p][0]);
                    acc[p][1] = fmaf(x[p][k], wv.y, acc[p][1]);
                    acc[p][2] = fmaf(x[p][k], wv.z, acc[p][2]);
                    acc[p][3] = fmaf(x[p][k], wv.w, acc[p][3]);
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            float v = acc[p][n];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            acc[p][n] = v;
        }
    if (lane < 16) {
        const int p = lane >> 2, n = lane & 3;
        const long long m = m0 + p;
        if (m < M && n < N) {
            float v = 0.f;
#pragma unroll
            for (int pp = 0; pp < 4; ++pp)
#pragma unroll
                for (int nn = 0; nn < 4; ++nn)
                    if (pp == p && nn == n) v = acc[pp][nn];
            const long long b = m / HW;
            out_nchw[(b * N + n) * HW + (m - b * HW)] = v + bias[n];
        }
    }
}

// planes [4 = (py, px)][B, H, W, C] -> out [B, 2H, 2W, C]: the four phase outputs of the up2 convolution interleaved into the image
// (16 bytes per thread; a pixel's C channels are one contiguous run on both sides)
__global__ void pixel_shuffle2_kernel(const float4* __restrict__ planes, int B, int H, int W, int C4, float4* __restrict__ out) {
    const long long n = (long long)B * H * W * 4 * C4;
    const long long plane = (long long)B * H * W * C4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int ox = (int)(r % (2 * W));
        r /= 2 * W;
        const int oy = (int)(r % (2 * H));
        const int b = (int)(r / (2 * H));
        const int phase = (oy & 1) * 2 + (ox & 1);
        out[i] = planes[phase * plane + (((long long)b * H + (oy >> 1)) * W + (ox >> 1)) * C4 + c];
    }
}

__global__ void avgpool2_kernel(const float* __restrict__ x, int B, int H, int W, int C, float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2;
    const long long n = (long long)B * Ho * Wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long r = i / C;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        const float* s = x + (((long long)b * H + 2 * oy) * W + 2 * ox) * C + c;
        // same summation order as ATen's avg_pool2d (row-major over the window), then divide
        out[i] = (s[0] + s[C] + s[(long long)W * C] + s[(long long)W * C + C]) / 4.f;
    }
}

__global__ void upsample2_kernel(const float* __restrict__ x, int B, int H, int W, int C, float* __restrict__ out) {
    const int Ho = H * 2, Wo = W * 2;
    const long long n = (long long)B * Ho * Wo * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long r = i / C;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        out[i] = x[(((long long)b * H + (oy >> 1)) * W + (ox >> 1)) * C + c];
    }
}

// 12-tap Kaiser-sinc low-pass (cutoff 0.25, half-width 0.3): alias_free_torch/filter.py:28-57 restated on the host
__constant__ float c_fir12[12];

static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

static void kaiser_sinc_filter12(float* out) {
    const int ks = 12, half = 6;
    const double cutoff = 0.25, half_width = 0.3, pi = 3.14159265358979323846;
    const double delta_f = 4.0 * half_width;
    const double A = 2.285 * (half - 1) * pi * delta_f + 7.95;
    double beta = 0.0;
    if (A > 50.0)
        beta = 0.1102 * (A - 8.7);
    else if (A >= 21.0)
        beta = 0.5842 * std::pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0);
    double f[12], sum = 0.0;
    for (int n = 0; n < ks; ++n) {
        const double r = (2.0 * n) / (ks - 1) - 1.0;                       // kaiser_window(periodic=False)
        const double w = bessel_i0(beta * std::sqrt(1.0 - r * r)) / bessel_i0(beta);
        const double t = (n - half) + 0.5;                                 // even kernel: arange(-6, 6) + 0.5
        const double xx = 2.0 * cutoff * t;
        const double sinc = xx == 0.0 ? 1.0 : std::sin(pi * xx) / (pi * xx);
        f[n] = 2.0 * cutoff * w * sinc;
        sum += f[n];
    }
    for (int n = 0; n < ks; ++n) out[n] = (float)(f[n] / sum);
}

// out[b,l,c] = sum_j f[j] * snake( up[2l + j - 5] ),  up[u] = 2 * sum_i f[.] x_rep[...]   (replicate edges)
//   UpSample1d : pad 5 replicate -> 2*conv_transpose(stride 2) -> crop [15:-15]       resample.py:25-33
//   DownSample1d: pad (5,6) replicate -> conv stride 2                                 filter.py:86-94
__global__ void snake_aa_kernel(const float* __restrict__ x, int B, int L, int C, const float* __restrict__ inv_beta,
                                const float* __restrict__ alpha, float* __restrict__ out) {
    const long long n = (long long)B * L * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long long r = i / C;
        const int l = (int)(r % L);
        const int b = (int)(r / L);
        const float* xs = x + (long long)b * L * C + c;
        const float al = alpha[c], ib = inv_beta[c];
        const int U = 2 * L;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            int u = 2 * l + j - 5;                 // index into the upsampled signal, replicate-clamped
            u = u < 0 ? 0 : (u >= U ? U - 1 : u);
            // upsampled[u] = 2 * sum_k f[k] * xpad[(u + 15 - k) / 2] for (u + 15 - k) even, xpad = replicate pad 5
            float up = 0.f;
            const int par = (u + 15) & 1;
#pragma unroll
            for (int k2 = 0; k2 < 6; ++k2) {
                const int k = 2 * k2 + par;
                int src = ((u + 15 - k) >> 1) - 5;
                src = src < 0 ? 0 : (src >= L ? L - 1 : src);
                up += c_fir12[k] * xs[(long long)src * C];
            }
            up *= 2.f;
            const float sn = sinf(up * al);
            acc += c_fir12[j] * (up + ib * sn * sn);
        }
        out[i] = acc;
    }
}

// The same Activation1d with every up-sampled, snake-activated value computed ONCE per tile instead of once per output
// tap that reads it (each is read by six outputs): a block owns 64 positions x CC channels, stages the x rows it needs
// (l0 - 6 .. l0 + 68, replicate-clamped) in LDS, forms snake(up[u]) for u = 2 l0 - 5 .. 2 l0 + 132 in LDS, then each thread
// applies the 12-tap down filter.  Per output: 2.2 sinf and ~25 FMAs instead of 12 sinf and ~84.  Arithmetic and summation
// order are those of snake_aa_kernel (bit-identical results).
template <int CC>
__global__ __launch_bounds__(256) void snake_aa_tiled_kernel(const float* __restrict__ x, int L, int C,
                                                             const float* __restrict__ inv_beta,
                                                             const float* __restrict__ alpha, float* __restrict__ out) {
    constexpr int TLO = 64, XR = TLO + 11, NU = 2 * TLO + 10, LANES = 256 / CC;
    __shared__ float xs[XR][CC];
    __shared__ float us[NU][CC];
    const int c = threadIdx.x % CC, s = threadIdx.x / CC;
    const int c0 = blockIdx.y * CC, l0 = blockIdx.x * TLO, b = blockIdx.z;
    const float* xb = x + (long long)b * L * C + c0 + c;
    for (int r = s; r < XR; r += LANES) {
        int src = l0 - 6 + r;
        src = src < 0 ? 0 : (src >= L ? L - 1 : src);
        xs[r][c] = xb[(long long)src * C];
    }
    __syncthreads();
    const float al = alpha[c0 + c], ib = inv_beta[c0 + c];
    const int U = 2 * L;
    for (int idx = s; idx < NU; idx += LANES) {
        int u = 2 * l0 - 5 + idx;
        u = u < 0 ? 0 : (u >= U ? U - 1 : u);
        float up = 0.f;
        const int par = (u + 15) & 1;
#pragma unroll
        for (int k2 = 0; k2 < 6; ++k2) {
            const int k = 2 * k2 + par;
            int src = ((u + 15 - k) >> 1) - 5;
            src = src < 0 ? 0 : (src >= L ? L - 1 : src);
            up += c_fir12[k] * xs[src - (l0 - 6)][c];
        }
        up *= 2.f;
        const float sn = sinf(up * al);
        us[idx][c] = up + ib * sn * sn;
    }
    __syncthreads();
    for (int q = s; q < TLO; q += LANES) {
        const int l = l0 + q;
        if (l < L) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 12; ++j) acc += c_fir12[j] * us[2 * q + j][c];
            out[((long long)b * L + l) * C + c0 + c] = acc;
        }
    }
}

// the two halves of a guided DDIM step's batch, cat([x] * 2), are one tensor until the first cross-attention (unet.cpp): the
// layers before it run on one half and this copy makes the [2B] tensor the rest of the network reads
__global__ void dup_half_kernel(const float4* __restrict__ x, long long n4, float4* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = x[i];
        out[i] = v;
        out[i + n4] = v;
    }
}

}  // namespace

void launch_timestep_embedding(const Ctx& ctx, const float* t, int B, int dim, float* out) {
    MAA_LAUNCH1(timestep_embedding_kernel, (long long)B * dim / 2, t, B, dim, out);
}
void launch_silu(const Ctx& ctx, const float* x, long long n, float* out) { MAA_LAUNCH1(silu_kernel, n, x, n, out); }
void launch_scale(const Ctx& ctx, const float* x, long long n, float s, float* out) {
    MAA_LAUNCH1(scale_kernel, n, x, n, s, out);
}
void launch_spec_from_mel(const Ctx& ctx, const float* mel, long long n, float* spec) {
    MAA_LAUNCH1(spec_from_mel_kernel, n, mel, n, spec);
}
void launch_nchw_to_nhwc(const Ctx& ctx, const float* x, int B, int C, int HW, float* out) {
    MAA_LAUNCH1(nchw_to_nhwc_kernel, (long long)B * C * HW, x, B, C, HW, out);
}
void launch_nhwc_to_nchw(const Ctx& ctx, const float* x, int B, int C, int HW, float* out, int ld_in) {
    MAA_LAUNCH1(nhwc_to_nchw_kernel, (long long)B * C * HW, x, B, C, HW, ld_in, out);
}
bool launch_narrow_conv3x3(const Ctx& ctx, const float* a_split, int lda, int B, int H, int W, int C, const float* w4, const float* bias,
                           int N, float* out_nchw) {
    const size_t lds = (size_t)9 * C * sizeof(float4);
    if (ctx.dtype != 1 || N > 4 || C % 32 != 0 || lds > 98304 || !w4 || !bias) return false;
    if (ctx.ws.dry) return true;
    const long long M = (long long)B * H * W;
    ProfScope prof(ctx, "narrow_conv3x3_kernel", 2.0 * M * N * 9.0 * C, 4.0 * M * C);
    ensure_dynamic_lds(reinterpret_cast<const void*>(narrow_conv3x3_kernel), ctx.device, (int)lds);
    hipLaunchKernelGGL(narrow_conv3x3_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), lds, ctx.stream, a_split, lda, B, H, W, C,
                       reinterpret_cast<const float4*>(w4), bias, N, out_nchw);
    MAA_HIP(hipGetLastError());
    return true;
}
void launch_pixel_shuffle2(const Ctx& ctx, const float* planes, int B, int H, int W, int C, float* out) {
    MAA_CHECK(C % 4 == 0, "pixel_shuffle2: channels must be a multiple of 4");
    MAA_LAUNCH1(pixel_shuffle2_kernel, (long long)B * H * W * C, reinterpret_cast<const float4*>(planes), B, H, W, C / 4,
                reinterpret_cast<float4*>(out));
}
void launch_dup_half(const Ctx& ctx, const float* x, long long n, float* out) {
    MAA_CHECK(n % 4 == 0, "dup_half: element count must be a multiple of 4");
    MAA_LAUNCH1(dup_half_kernel, n / 4, reinterpret_cast<const float4*>(x), n / 4, reinterpret_cast<float4*>(out));
}
void launch_avgpool2(const Ctx& ctx, const float* x, int B, int H, int W, int C, float* out) {
    MAA_LAUNCH1(avgpool2_kernel, (long long)B * (H / 2) * (W / 2) * C, x, B, H, W, C, out);
}
void launch_upsample2(const Ctx& ctx, const float* x, int B, int H, int W, int C, float* out) {
    MAA_LAUNCH1(upsample2_kernel, (long long)B * H * W * C * 4, x, B, H, W, C, out);
}

static std::once_flag g_fir_once[64];      // one upload of the FIR taps per device (thread-safe: contexts on several threads)
void launch_snake_aa(const Ctx& ctx, const float* x, int B, int L, int C, const float* inv_beta, const float* alpha,
                     float* out) {
    if (ctx.ws.dry) return;
    MAA_CHECK(ctx.device >= 0 && ctx.device < 64, "device index");
    std::call_once(g_fir_once[ctx.device], [] {
        float f[12];
        kaiser_sinc_filter12(f);
        MAA_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_fir12), f, sizeof(f)));
    });
    if ((C % 64 == 0 || C == 32) && B <= 65535) {
        ProfScope prof(ctx, "snake_aa_kernel", 0.0, 8.0 * (double)B * L * C);
        const dim3 grid((unsigned)((L + 63) / 64), (unsigned)(C % 64 == 0 ? C / 64 : 1), (unsigned)B);
        if (C % 64 == 0)
            hipLaunchKernelGGL(snake_aa_tiled_kernel<64>, grid, dim3(256), 0, ctx.stream, x, L, C, inv_beta, alpha, out);
        else
            hipLaunchKernelGGL(snake_aa_tiled_kernel<32>, grid, dim3(256), 0, ctx.stream, x, L, C, inv_beta, alpha, out);
        MAA_HIP(hipGetLastError());
        return;
    }
    MAA_LAUNCH1(snake_aa_kernel, (long long)B * L * C, x, B, L, C, inv_beta, alpha, out);
}

}  // namespace maa
