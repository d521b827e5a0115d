// Crop-and-stitch of `split_input_params` (LatentDiffusion_audio.apply_model, ldm/models/diffusion/ddpm_audio.py:572-654): the
// two passes around the UNet when a latent wider than the training size is evaluated as overlapping crops.
//   unfold  x [nB, C, H, W] -> crop rows [nB * L, C, kh, kw], crop l = ly * Lx + lx at (ly * sh, lx * sw): torch.nn.Unfold's
//           column order (:582-585), a copy
//   fold    out[n, c, Y, X] = (sum_l w[p, l] * e[n * L + l, c, p]) / norm[Y, X] over the crops that cover (Y, X), ascending l,
//           p = (Y - ly * sh) * kw + (X - lx * sw): `o * weighting`, torch.nn.Fold and `/ normalization` (:649-654) as a gather --
//           no atomics, one fixed summation order
//   norm    norm[Y, X] = sum_l w[p, l] over the same crops (get_fold_unfold's fold(weighting), :260), summed in fp64 and rounded once
// The weighting is held transposed, wT [L][kh * kw], so that a crop's weights are contiguous along the crop's rows like its eps.
// All three are one coalesced pass over a few hundred kilobytes; 16-byte accesses along W where kw, sw and W are multiples of 4
// (then four neighbouring columns lie in the same crops and every row starts 16-byte aligned).
#include "elementwise_launch.h"

namespace maa {
namespace {

struct SplitGeom {
    int C, H, W, kh, kw, sh, sw, Ly, Lx;
};

template <int V>
struct Vec {
    float v[V];
};
template <int V>
__device__ inline Vec<V> load_vec(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V>
__device__ inline void store_vec(float* p, const Vec<V>& r) {
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
        *p = r.v[0];
}

// first and last crop index along one axis that covers position `pos` (crop i spans [i * s, i * s + k))
__device__ inline void covering(int pos, int k, int s, int n, int& lo, int& hi) {
    lo = pos < k ? 0 : (pos - k + s) / s;
    hi = pos / s;
    if (hi > n - 1) hi = n - 1;
}

template <int V>
__global__ void split_unfold_kernel(const float* __restrict__ x, SplitGeom g, long long nv, float* __restrict__ out) {
    const int kwv = g.kw / V, L = g.Ly * g.Lx;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int xv = (int)(r % kwv);
        r /= kwv;
        const int y = (int)(r % g.kh);
        r /= g.kh;
        const int c = (int)(r % g.C);
        r /= g.C;
        const int l = (int)(r % L);
        const long long n = r / L;
        const int ly = l / g.Lx, lx = l - ly * g.Lx;
        const long long src = ((n * g.C + c) * g.H + ly * g.sh + y) * (long long)g.W + lx * g.sw + xv * V;
        store_vec<V>(out + i * V, load_vec<V>(x + src));
    }
}

template <int V>
__global__ void split_fold_kernel(const float* __restrict__ e, const float* __restrict__ wT, const float* __restrict__ norm,
                                  SplitGeom g, long long nv, float* __restrict__ out) {
    const int Wv = g.W / V, L = g.Ly * g.Lx, kk = g.kh * g.kw;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        const int X = (int)(r % Wv) * V;
        r /= Wv;
        const int Y = (int)(r % g.H);
        r /= g.H;
        const int c = (int)(r % g.C);
        const long long n = r / g.C;
        int ly0, ly1, lx0, lx1;
        covering(Y, g.kh, g.sh, g.Ly, ly0, ly1);
        covering(X, g.kw, g.sw, g.Lx, lx0, lx1);      // (V == 4: the same crops cover X .. X + 3)
        Vec<V> acc;
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
        for (int ly = ly0; ly <= ly1; ++ly)
            for (int lx = lx0; lx <= lx1; ++lx) {
                const int l = ly * g.Lx + lx;
                const int p = (Y - ly * g.sh) * g.kw + (X - lx * g.sw);
                const Vec<V> ev = load_vec<V>(e + ((n * L + l) * g.C + c) * (long long)kk + p);
                const Vec<V> wv = load_vec<V>(wT + (long long)l * kk + p);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float t = wv.v[k] * ev.v[k];
                    acc.v[k] = acc.v[k] + t;
                }
            }
        const Vec<V> nv4 = load_vec<V>(norm + (long long)Y * g.W + X);
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = acc.v[k] / nv4.v[k];
        store_vec<V>(out + i * V, acc);
    }
}

__global__ void split_norm_kernel(const float* __restrict__ wT, SplitGeom g, float* __restrict__ norm) {
    const int kk = g.kh * g.kw, n = g.H * g.W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int Y = i / g.W, X = i - Y * g.W;
        int ly0, ly1, lx0, lx1;
        covering(Y, g.kh, g.sh, g.Ly, ly0, ly1);
        covering(X, g.kw, g.sw, g.Lx, lx0, lx1);
        double s = 0.0;
        for (int ly = ly0; ly <= ly1; ++ly)
            for (int lx = lx0; lx <= lx1; ++lx)
                s += (double)wT[(long long)(ly * g.Lx + lx) * kk + (Y - ly * g.sh) * g.kw + (X - lx * g.sw)];
        norm[i] = (float)s;
    }
}

// src [rows][len] -> dst [rows * rep][len]: row r of src is written to rows r * rep .. r * rep + rep - 1 of dst
template <int V>
__global__ void repeat_rows_kernel(const float* __restrict__ src, long long lenv, int rep, long long nv, float* __restrict__ dst) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / lenv, k = i - row * lenv;
        store_vec<V>(dst + i * V, load_vec<V>(src + ((row / rep) * lenv + k) * V));
    }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

SplitGeom geom(int C, int H, int W, int kh, int kw, int sh, int sw) {
    split_check(H, W, kh, kw, sh, sw);
    MAA_CHECK(C > 0, "split: no channels");
    SplitGeom g;
    g.C = C, g.H = H, g.W = W, g.kh = kh, g.kw = kw, g.sh = sh, g.sw = sw;
    g.Ly = (H - kh) / sh + 1, g.Lx = (W - kw) / sw + 1;
    return g;
}

}  // namespace

void split_check(int H, int W, int kh, int kw, int sh, int sw) {
    MAA_CHECK(H > 0 && W > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0, "split: sizes, ks and stride must be positive");
    MAA_CHECK(kh <= H && kw <= W, "split: ks is larger than the latent (ddpm_audio.py:250-251 counts no crop)");
    MAA_CHECK(sh <= kh && sw <= kw, "split: a stride larger than ks leaves gaps between the crops");
    MAA_CHECK((H - kh) % sh == 0 && (W - kw) % sw == 0,
              "split: ks and stride leave part of the latent in no crop (Fold leaves it at 0 and ddpm_audio.py:654 divides 0 by 0)");
}

int split_crops(int H, int W, int kh, int kw, int sh, int sw) {
    split_check(H, W, kh, kw, sh, sw);
    return ((H - kh) / sh + 1) * ((W - kw) / sw + 1);
}

void launch_split_unfold(const Ctx& ctx, const float* x, int nB, int C, int H, int W, int kh, int kw, int sh, int sw, float* out) {
    const SplitGeom g = geom(C, H, W, kh, kw, sh, sw);
    MAA_CHECK(nB > 0 && x && out, "split unfold: empty problem");
    if (ctx.ws.dry) return;
    const long long n = (long long)nB * g.Ly * g.Lx * C * kh * kw;
    ProfScope prof(ctx, "split_unfold_kernel", 0.0, 8.0 * (double)n);
    if (kw % 4 == 0 && sw % 4 == 0 && W % 4 == 0 && al16(x) && al16(out))
        hipLaunchKernelGGL(split_unfold_kernel<4>, grid_for(n / 4, 4096), dim3(256), 0, ctx.stream, x, g, n / 4, out);
    else
        hipLaunchKernelGGL(split_unfold_kernel<1>, grid_for(n, 4096), dim3(256), 0, ctx.stream, x, g, n, out);
    MAA_HIP(hipGetLastError());
}

void launch_split_norm(const Ctx& ctx, const float* wT, int H, int W, int kh, int kw, int sh, int sw, float* norm) {
    const SplitGeom g = geom(1, H, W, kh, kw, sh, sw);
    MAA_CHECK(wT && norm, "split norm: empty problem");
    if (ctx.ws.dry) return;
    ProfScope prof(ctx, "split_norm_kernel", 0.0, 4.0 * (double)H * W);
    hipLaunchKernelGGL(split_norm_kernel, grid_for((long long)H * W, 4096), dim3(256), 0, ctx.stream, wT, g, norm);
    MAA_HIP(hipGetLastError());
}

void launch_split_fold(const Ctx& ctx, const float* e, const float* wT, const float* norm, int nB, int C, int H, int W, int kh,
                       int kw, int sh, int sw, float* out) {
    const SplitGeom g = geom(C, H, W, kh, kw, sh, sw);
    MAA_CHECK(nB > 0 && e && wT && norm && out, "split fold: empty problem");
    if (ctx.ws.dry) return;
    const long long n = (long long)nB * C * H * W;
    ProfScope prof(ctx, "split_fold_kernel", 2.0 * (double)nB * g.Ly * g.Lx * C * kh * kw,
                   4.0 * ((double)n + 2.0 * (double)nB * g.Ly * g.Lx * C * kh * kw));
    if (kw % 4 == 0 && sw % 4 == 0 && W % 4 == 0 && al16(e) && al16(wT) && al16(norm) && al16(out))
        hipLaunchKernelGGL(split_fold_kernel<4>, grid_for(n / 4, 4096), dim3(256), 0, ctx.stream, e, wT, norm, g, n / 4, out);
    else
        hipLaunchKernelGGL(split_fold_kernel<1>, grid_for(n, 4096), dim3(256), 0, ctx.stream, e, wT, norm, g, n, out);
    MAA_HIP(hipGetLastError());
}

void launch_repeat_rows(const Ctx& ctx, const float* src, long long rows, long long len, int rep, float* dst) {
    MAA_CHECK(rows > 0 && len > 0 && rep > 0 && src && dst, "repeat_rows: empty problem");
    if (ctx.ws.dry) return;
    const long long n = rows * rep * len;
    ProfScope prof(ctx, "repeat_rows_kernel", 0.0, 8.0 * (double)n);
    if (len % 4 == 0 && al16(src) && al16(dst))
        hipLaunchKernelGGL(repeat_rows_kernel<4>, grid_for(n / 4, 4096), dim3(256), 0, ctx.stream, src, len / 4, rep, n / 4, dst);
    else
        hipLaunchKernelGGL(repeat_rows_kernel<1>, grid_for(n, 4096), dim3(256), 0, ctx.stream, src, len, rep, n, dst);
    MAA_HIP(hipGetLastError());
}

}  // namespace maa
