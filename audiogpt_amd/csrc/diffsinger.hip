// Elementwise kernels of DiffSinger's denoiser (DiffNet), channels-last [B, T, C].  (The step kernels of its two sampling loops
// are in sampler_steps.hip.)
//
// Replaces (NeuralSeq/modules/diff/): net.py:31-44 SinusoidalPosEmb, diffusion.py:68-70 Mish, net.py:68-81 the gated
// activation and the residual / skip bookkeeping of ResidualBlock.
#include "elementwise_launch.h"

namespace maa {

namespace {

// [sin | cos] of t * exp(-ln(1e4) * j / (half - 1))      (net.py:36-44)
__global__ void ds_pos_emb_kernel(const float* __restrict__ t, int B, int dim, float* __restrict__ out) {
    const int half = dim / 2;
    const float scale = 9.210340371976184f / (float)(half - 1);          // math.log(10000) / (half_dim - 1)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * half; i += gridDim.x * blockDim.x) {
        const int b = i / half, j = i - b * half;
        const float f = expf((float)j * -scale);
        const float a = t[b] * f;
        out[(long long)b * dim + j] = sinf(a);
        out[(long long)b * dim + half + j] = cosf(a);
    }
}

// x * tanh(softplus(x)), softplus with torch's threshold 20 (F.softplus default)
__global__ void ds_mish_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = x[i];
        const float sp = v > 20.f ? v : log1pf(expf(v));
        out[i] = v * tanhf(sp);
    }
}

// out[b, t, c] = x[b, t, c] + step[b, c]       (net.py:71-73: y = x + diffusion_step, broadcast over time)
__global__ void ds_add_step_kernel(const float* __restrict__ x, const float* __restrict__ step, int ld_step, long long rows,
                                   int T, int C, float* __restrict__ out) {
    const long long n = rows * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C;
        const int c = (int)(i - r * C);
        out[i] = x[i] + step[(r / T) * ld_step + c];
    }
}

// gate, filter = chunk(y, 2, dim = channels); z = sigmoid(gate) * tanh(filter)      (net.py:76-77)
__global__ void ds_gate_kernel(const float* __restrict__ y, long long rows, int C, float* __restrict__ z) {
    const long long n = rows * C;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C;
        const int c = (int)(i - r * C);
        const float g = y[r * 2 * C + c], f = y[r * 2 * C + C + c];
        z[i] = (1.f / (1.f + expf(-g))) * tanhf(f);
    }
}

// residual, skip = chunk(y2, 2); x = (x + residual) / sqrt(2); skip_sum (+)= skip; xin = x + next_step[b]   (net.py:79-81)
__global__ void ds_residual_kernel(const float* __restrict__ y2, long long rows, int T, int C, float* __restrict__ x,
                                   float* __restrict__ skip, int first, const float* __restrict__ next_step, int ld_step,
                                   float* __restrict__ xin) {
    const long long n = rows * C;
    const float rs2 = 1.41421356237309504880f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / C;
        const int c = (int)(i - r * C);
        const float xn = (x[i] + y2[r * 2 * C + c]) / rs2;
        x[i] = xn;
        const float s = y2[r * 2 * C + C + c];
        skip[i] = first ? s : skip[i] + s;
        if (next_step) xin[i] = xn + next_step[(r / T) * ld_step + c];
    }
}

__global__ void ds_fill_kernel(float* __restrict__ p, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

void launch_ds_pos_emb(const Ctx& ctx, const float* t, int B, int dim, float* out) {
    MAA_LAUNCH1(ds_pos_emb_kernel, (long long)B * dim / 2, t, B, dim, out);
}
void launch_ds_mish(const Ctx& ctx, const float* x, long long n, float* out) { MAA_LAUNCH1(ds_mish_kernel, n, x, n, out); }
void launch_ds_add_step(const Ctx& ctx, const float* x, const float* step, int ld_step, long long rows, int T, int C,
                        float* out) {
    MAA_LAUNCH1(ds_add_step_kernel, rows * C, x, step, ld_step, rows, T, C, out);
}
void launch_ds_gate(const Ctx& ctx, const float* y, long long rows, int C, float* z) {
    MAA_LAUNCH1(ds_gate_kernel, rows * C, y, rows, C, z);
}
void launch_ds_residual(const Ctx& ctx, const float* y2, long long rows, int T, int C, float* x, float* skip, int first,
                        const float* next_step, int ld_step, float* xin) {
    MAA_LAUNCH1(ds_residual_kernel, rows * C, y2, rows, T, C, x, skip, first, next_step, ld_step, xin);
}
void launch_ds_fill(const Ctx& ctx, float* p, int n, float v) {
    if (ctx.ws.dry) return;
    hipLaunchKernelGGL(ds_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx.stream, p, n, v);
    MAA_HIP(hipGetLastError());
}

}  // namespace maa
