// GroupNorm(32) [+SiLU], LayerNorm and row softmax for channels-last fp32 activations (gfx950).
//   GroupNorm32 / Normalize: ldm/modules/diffusionmodules/util.py:199-216 (eps 1e-5),
//       ldm/modules/attention.py:76-77 and diffusionmodules/model.py:38-39 (eps 1e-6), swish model.py:33-35
//   LayerNorm: ldm/modules/attention.py:203-205 (eps 1e-5)
//   softmax:   ldm/modules/attention.py:188, openaimodel.py:370, model.py:191
// All three are HBM/L2-bound; reductions are wave64 shuffles plus one LDS hop across the 4 waves.
#include "igemm_device.h"
#include "maa_internal.h"
#include "row_device.h"

namespace maa {
namespace {

// the waves' sums added left to right over blockDim / 64 waves (not pitch.hip's (r0 + r1) + (r2 + r3): another rounding, so the
// two stay apart)
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

// write 4 consecutive channels (c % 4 == 0) of row `row` either as fp32 or in the "split32" form read by the bf16
// GEMM engine: every 32 channels of a row take one 128-byte line [32 bf16 hi | 32 bf16 lo], hi = bf16(v),
// lo = bf16(v - hi); the row pitch is the same C*4 bytes as fp32
__device__ __forceinline__ void store4(float* out, long long row, int c, int C, int split, float4 v) {
    if (!split) {
        *reinterpret_cast<float4*>(out + row * C + c) = v;
        return;
    }
    unsigned short* o = reinterpret_cast<unsigned short*>(out) + row * C * 2 + (c >> 5) * 64 + (c & 31);
    uint2 hi, lo;
    split2(v.x, v.y, hi.x, lo.x);
    split2(v.z, v.w, hi.y, lo.y);
    *reinterpret_cast<uint2*>(o) = hi;
    *reinterpret_cast<uint2*>(o + 32) = lo;
}

// GroupNorm pass 1: one block per (sample, group) -> tab[(b*C + c)*2] = {scale, shift} for the group's channels
// (scale = gamma*rstd, shift = beta - mean*scale, as ATen forms them); threads = (position
// lane, channel-in-group).  One pass over the data: sums of d = x - pivot and d*d, eight independent loads in flight per
// thread.  The pivot is the block-reduced mean of the group's first slab -- the first 8 * tp_n positions x cpg channels, up
// to 2048 elements, which are each thread's first eight loads and stay in registers across the reduction -- so no single
// element (the group's first one sits in a corner pixel next to the zero padding) and no single position decides how much
// var = E[d^2] - E[d]^2 cancels: a whole position at 50 sigma moves this pivot by 50 / (8 tp_n) <= 6.3 sigma (cpg <= 256),
// one element at 1000 sigma by 1000 / (8 tp_n cpg) <= 0.6 sigma.  Fixed reduction order: results are bit-reproducible.
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x1, int ld1, int C1,
                                                       const float* __restrict__ x2, int ld2, int C2, int HW,
                                                       int groups, float eps, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ tab) {
    __shared__ float red[4];
    __shared__ float mr[2];
    const int C = C1 + C2, cpg = C / groups;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
    const int tp_n = 256 / cpg;
    const int tc = threadIdx.x % cpg, tp = threadIdx.x / cpg;
    const bool active = tp < tp_n;
    const int c = g * cpg + tc;
    const float* src;
    long long ld;
    if (c < C1) {
        src = x1 + (long long)b * HW * ld1 + c;
        ld = ld1;
    } else {
        src = x2 + (long long)b * HW * ld2 + (c - C1);
        ld = ld2;
    }
    const int c0 = g * cpg;
    const float n = (float)HW * (float)cpg;
    // eight independent loads in flight per thread: the pass is latency-bound (a 10 x 78 level is 31 positions per thread)
    constexpr int U = 8;
    float d[U], sa[U], qa[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int pu = tp + u * tp_n;
        d[u] = active && pu < HW ? src[(long long)pu * ld] : 0.f;
        sa[u] = qa[u] = 0.f;
    }
    const int slab = HW < U * tp_n ? HW : U * tp_n;       // positions of the first slab
    const float pivot = block_sum(((d[0] + d[4]) + (d[1] + d[5])) + ((d[2] + d[6]) + (d[3] + d[7])), red) / ((float)slab * (float)cpg);
    if (active) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (tp + u * tp_n < HW) {
                d[u] -= pivot;
                sa[u] = d[u];
                qa[u] = d[u] * d[u];
            }
        for (int pos = tp + U * tp_n; pos < HW; pos += U * tp_n) {          // a position past the end reads as the pivot: d = 0
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pu = pos + u * tp_n;
                d[u] = pu < HW ? src[(long long)pu * ld] : pivot;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] -= pivot;
                sa[u] += d[u];
                qa[u] += d[u] * d[u];
            }
        }
    }
    const float s0 = sa[0] + sa[4], s1 = sa[1] + sa[5], s2 = sa[2] + sa[6], s3 = sa[3] + sa[7];
    const float q0 = qa[0] + qa[4], q1 = qa[1] + qa[5], q2 = qa[2] + qa[6], q3 = qa[3] + qa[7];
    const float sm = block_sum((s0 + s1) + (s2 + s3), red) / n;
    const float qm = block_sum((q0 + q1) + (q2 + q3), red) / n;
    if (threadIdx.x == 0) {
        const float var = fmaxf(qm - sm * sm, 0.f);
        mr[0] = pivot + sm;
        mr[1] = 1.f / sqrtf(var + eps);
    }
    __syncthreads();
    if ((int)threadIdx.x < cpg) {
        const int cc = c0 + threadIdx.x;
        const float sc = gamma[cc] * mr[1];
        tab[2 * ((long long)b * C + cc)] = sc;
        tab[2 * ((long long)b * C + cc) + 1] = beta[cc] - mr[0] * sc;
    }
}

// GroupNorm pass 2: y = x*scale + shift [+ SiLU].  Block = 16 rows of one sample x all channels, thread = (row lane,
// channel-quad lane): the per-(sample, channel) scale/shift pair is fetched once per quad and reused down the rows;
// 16 quad lanes = 256 contiguous bytes per row, fp32 or split32 out.
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x1, int ld1, int C1,
                                                       const float* __restrict__ x2, int ld2, int C2, int HW,
                                                       const float* __restrict__ tab, int silu,
                                                       float* __restrict__ out, int split, float* __restrict__ raw_split) {
    const int C = C1 + C2, c4n = C >> 2;
    const int b = blockIdx.y, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r0 = blockIdx.x * 16 + ty;
    if (r0 >= HW) return;
    const long long row = (long long)b * HW + r0;
    const float4* t4 = reinterpret_cast<const float4*>(tab + 2 * (long long)b * C);
    for (int q = tx + 16 * blockIdx.z; q < c4n; q += 16 * gridDim.z) {      // grid.z splits the quads of small tensors
        const int c = q * 4;
        const float4 ta = t4[2 * q], tb = t4[2 * q + 1];      // {sc0, sh0, sc1, sh1}, {sc2, sh2, sc3, sh3}
        const float4 v = c < C1 ? *reinterpret_cast<const float4*>(x1 + row * ld1 + c)
                                : *reinterpret_cast<const float4*>(x2 + row * ld2 + (c - C1));
        float4 y;
        y.x = v.x * ta.x + ta.y;
        y.y = v.y * ta.z + ta.w;
        y.z = v.z * tb.x + tb.y;
        y.w = v.w * tb.z + tb.w;
        if (silu) {
            y.x = __fdividef(y.x, 1.f + __expf(-y.x));
            y.y = __fdividef(y.y, 1.f + __expf(-y.y));
            y.z = __fdividef(y.z, 1.f + __expf(-y.z));
            y.w = __fdividef(y.w, 1.f + __expf(-y.w));
        }
        store4(out, row, c, C, split, y);
        // second output: the UN-normalised row as split32 (the ResBlock's 1x1 skip convolution reads the same (h | skip) rows:
        // with this copy both of its operands reach LDS by DMA instead of through the register-staged engine)
        if (raw_split) store4(raw_split, row, c, C, 1, v);
    }
}


// GroupNorm in ONE pass over the data (round 5): a workgroup owns GPB consecutive groups of one sample -- CB = GPB cpg channels,
// a run of CB * 4 contiguous bytes per position -- and keeps all of that sample's rows of them in registers: thread (row lane ty,
// float4 column tx) loads rows ty, ty + RL, ... (NR float4s, all in flight together), the statistics are reduced through LDS in a
// fixed order, and the normalised (+ SiLU) rows are written from the registers -- fp32 or split32, plus the optional raw split32
// copy -- so the tensor is read once and the statistics launch, its table and the dependent second launch are gone (two launches
// of 10 + 8 us per GroupNorm at the UNet's sizes, both latency-bound: DESIGN.md 3.4).  With the rows in registers the statistics
// are the exact two-pass ones: the group sums are reduced to the mean, the mean is broadcast, and the squares of x - mean are
// reduced the same way (no pivot: the variance does not depend on any one element or position being typical of its group).
// Then scale = gamma rstd, shift = beta - mean scale, y = x scale + shift, as in the two-launch kernels.  The layout (GPB, RL, NR)
// is a function of (C, HW) only and a workgroup sees one sample: a sample's result does not depend on its batch.
//
// One LDS reduction of a per-thread float4 of partials (red[t]) to per-group totals (gtot[0 .. GPB)), every step in a fixed order:
// thread (half h, channel cc) adds half of the RL row lanes' partials of its channel in four interleaved chains, then one thread
// per group adds its 2 cpg column sums.  Starts and ends with a barrier.
__device__ __forceinline__ void gn_group_reduce(float* red, float* colsum, float* gtot, float4 part, int t, int RL, int Q, int CB,
                                                int GPB, int cpg) {
    *reinterpret_cast<float4*>(red + (size_t)t * 4) = part;
    __syncthreads();
    if (t < 2 * CB) {
        const int h = t / CB, cc = t - h * CB, RLh = (RL + 1) >> 1;
        const int y1 = h ? RL : RLh;
        const float* p0 = red + cc;                      // channel cc of row lane y: red[(y Q + cc / 4) 4 + cc % 4]
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int y = h ? RLh : 0;
        for (; y + 3 < y1; y += 4) {
            a0 += p0[(size_t)(y + 0) * Q * 4];
            a1 += p0[(size_t)(y + 1) * Q * 4];
            a2 += p0[(size_t)(y + 2) * Q * 4];
            a3 += p0[(size_t)(y + 3) * Q * 4];
        }
        for (; y < y1; ++y) a0 += p0[(size_t)y * Q * 4];
        colsum[t] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    if (t < GPB) {
        float s = 0.f;
        for (int i = 0; i < cpg; ++i) s += colsum[t * cpg + i] + colsum[CB + t * cpg + i];
        gtot[t] = s;
    }
    __syncthreads();
}

template <int NR>
__global__ __launch_bounds__(1024) void gn_fused_kernel(const float* __restrict__ x1, int ld1, int C1,
                                                        const float* __restrict__ x2, int ld2, int C2, int HW, int groups,
                                                        int GPB, float eps, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int silu, float* __restrict__ out,
                                                        int split, float* __restrict__ raw_split, int nblk) {
    extern __shared__ float gsm[];      // red[RL Q 4] | colsum[2 CB] | gsum[GPB] | gsq[GPB]
    const int C = C1 + C2, cpg = C / groups, CB = GPB * cpg, Q = CB >> 2;
    const int RL = (int)blockDim.x / Q;                      // (blockDim.x == RL Q)
    // work item = (sample, group block), sample-major; XCD-contiguous: a sample's rows are read and written on the XCD whose
    // igemm tiles produce / consume them
    const int w = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int b = w / nblk, c_lo = (w - b * nblk) * CB;
    const int t = threadIdx.x, ty = t / Q, tx = t - ty * Q;
    const int c = c_lo + 4 * tx;
    float* const red = gsm;
    float* const colsum = gsm + (size_t)RL * Q * 4;
    float* const gsum = colsum + 2 * CB;
    float* const gsq = gsum + GPB;
    const float* src;
    long long ld;
    if (c < C1) {
        src = x1 + (long long)b * HW * ld1 + c;
        ld = ld1;
    } else {
        src = x2 + (long long)b * HW * ld2 + (c - C1);
        ld = ld2;
    }
    // group (within the block) of each of the float4's four channels: one float4 can span two groups
    int gl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gl[j] = (4 * tx + j) / cpg;
    float4 v[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int r = ty + RL * k;
        v[k] = r < HW ? *reinterpret_cast<const float4*>(src + (long long)r * ld) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float n = (float)HW * (float)cpg;
    float4 sd = make_float4(0.f, 0.f, 0.f, 0.f);      // a row past the end was loaded as 0
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        sd.x += v[k].x;
        sd.y += v[k].y;
        sd.z += v[k].z;
        sd.w += v[k].w;
    }
    gn_group_reduce(red, colsum, gsum, sd, t, RL, Q, CB, GPB, cpg);
    float mu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mu[j] = gsum[gl[j]] / n;
    float4 qd = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < NR; ++k)
        if (ty + RL * k < HW) {
            const float d0 = v[k].x - mu[0], d1 = v[k].y - mu[1], d2 = v[k].z - mu[2], d3 = v[k].w - mu[3];
            qd.x += d0 * d0;
            qd.y += d1 * d1;
            qd.z += d2 * d2;
            qd.w += d3 * d3;
        }
    gn_group_reduce(red, colsum, gsq, qd, t, RL, Q, CB, GPB, cpg);
    float sc[4], sh[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float var = fmaxf(gsq[gl[j]] / n, 0.f);
        sc[j] = gamma[c + j] * (1.f / sqrtf(var + eps));
        sh[j] = beta[c + j] - mu[j] * sc[j];
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int r = ty + RL * k;
        if (r < HW) {
            const long long row = (long long)b * HW + r;
            float4 y;
            y.x = v[k].x * sc[0] + sh[0];
            y.y = v[k].y * sc[1] + sh[1];
            y.z = v[k].z * sc[2] + sh[2];
            y.w = v[k].w * sc[3] + sh[3];
            if (silu) {
                y.x = __fdividef(y.x, 1.f + __expf(-y.x));
                y.y = __fdividef(y.y, 1.f + __expf(-y.y));
                y.z = __fdividef(y.z, 1.f + __expf(-y.z));
                y.w = __fdividef(y.w, 1.f + __expf(-y.w));
            }
            store4(out, row, c, C, split, y);
            if (raw_split) store4(raw_split, row, c, C, 1, v[k]);
        }
    }
}

// Layout of the one-pass GroupNorm for a tensor of C channels x HW positions per sample, or gpb = 0 when a sample's rows of
// even one group block do not fit the registers of a workgroup (the VAE's large images: the two-pass kernels stay).  A function
// of (C, HW, groups) only.
struct GnFusedPlan {
    int gpb = 0, nr = 0, threads = 0;
    size_t lds = 0;
};
GnFusedPlan gn_fused_plan(int C, int C1, int HW, int groups) {
    GnFusedPlan pl;
    const int cpg = C / groups;
    // at most eight float4 rows per thread where some block width allows it (no register pressure at 1024 threads), else
    // twelve, else sixteen (which spills a little); wider blocks (longer contiguous runs per position) first
    for (int cap : {8, 12, 16})
        for (int gpb : {4, 2, 8, 1, 16}) {
            if (groups % gpb) continue;
            const int CB = gpb * cpg;
            if (CB % 4 || CB > 512) continue;
            const int Q = CB / 4, RL = 1024 / Q;
            if (RL < 1) continue;
            const int need = (HW + RL - 1) / RL;
            if (need > cap) continue;
            pl.gpb = gpb;
            pl.nr = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : need <= 12 ? 12 : 16;
            pl.threads = RL * Q;
            pl.lds = ((size_t)RL * Q * 4 + 2 * CB + 2 * gpb) * sizeof(float);
            return pl;
        }
    return pl;
}

// LayerNorm: one wave per row, four channels per lane per step, row cached in registers (C <= 256*NR): row_device.h's LnRow
template <int NR>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, long long rows, int C,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        float* __restrict__ out, int split) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)xcd_contiguous((int)blockIdx.x, (int)gridDim.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    LnRow<NR> r;
    r.load(x + row * C, C, lane, eps);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < C) store4(out, row, c, C, split, r.norm(i, c, gamma, beta));
    }
}

// one wave per row; NR > 0: row cached in registers, NR == 0: three passes over memory
// causal_nq > 0: row r belongs to query r % causal_nq, which sees keys 0 .. that index only (the rest are written as 0)
template <int NR>
__global__ __launch_bounds__(256) void softmax_kernel(float* __restrict__ s, long long rows, int cols, int ld, int causal_nq) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* p = s + row * ld;
    if (causal_nq > 0) {
        const int q = (int)(row % causal_nq);
        cols = cols < q + 1 ? cols : q + 1;
    }
    if constexpr (NR > 0) {
        float v[NR];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < cols ? p[c] : -INFINITY;
            m = fmaxf(m, v[i]);
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < cols ? expf(v[i] - m) : 0.f;
            sum += v[i];
        }
        const float inv = 1.f / wave_sum(sum);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int c = lane + 64 * i;
            if (c < ld) p[c] = c < cols ? v[i] * inv : 0.f;
        }
    } else {
        float m = -INFINITY;
        for (int c = lane; c < cols; c += 64) m = fmaxf(m, p[c]);
        m = wave_max(m);
        float sum = 0.f;
        for (int c = lane; c < cols; c += 64) {
            const float e = expf(p[c] - m);
            p[c] = e;
            sum += e;
        }
        const float inv = 1.f / wave_sum(sum);
        for (int c = lane; c < ld; c += 64) p[c] = c < cols ? p[c] * inv : 0.f;
    }
}

// softmax_kernel<0> with a key mask of the row's sample: three passes over memory, a hidden column counts as -inf
__global__ __launch_bounds__(256) void softmax_masked_kernel(float* __restrict__ s, long long rows, int cols, int ld,
                                                             const float* __restrict__ key_mask, long long rows_per_sample) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* p = s + row * ld;
    const float* hid = key_mask + (row / rows_per_sample) * cols;
    float m = -INFINITY;
    for (int c = lane; c < cols; c += 64) m = fmaxf(m, hid[c] != 0.f ? -INFINITY : p[c]);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < cols; c += 64) {
        const float e = hid[c] != 0.f || m == -INFINITY ? 0.f : expf(p[c] - m);
        p[c] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
    for (int c = lane; c < ld; c += 64) p[c] = c < cols ? p[c] * inv : 0.f;
}

// fp32 rows -> split32 rows (same pitch): what a normalisation with out_split = 1 does to its result, on its own
// (slope != 1: leaky-relu first -- the pre-activated input of the vocoders' first MRF convolution)
__global__ __launch_bounds__(256) void split32_pack_kernel(const float* __restrict__ x, long long rows, int C, float slope,
                                                           float* __restrict__ out) {
    const long long n4 = rows * (C / 4);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long row = i / (C / 4);
        const int c = (int)(i - row * (C / 4)) * 4;
        float4 v = *reinterpret_cast<const float4*>(x + row * C + c);
        v.x = v.x > 0.f ? v.x : v.x * slope;
        v.y = v.y > 0.f ? v.y : v.y * slope;
        v.z = v.z > 0.f ? v.z : v.z * slope;
        v.w = v.w > 0.f ? v.w : v.w * slope;
        store4(out, row, c, C, 1, v);
    }
}

// split32 rows -> fp32 rows (hi + lo): tests of the kernels that only emit the split form
__global__ __launch_bounds__(256) void split32_unpack_kernel(const float* __restrict__ x, long long rows, int C, float* __restrict__ out) {
    const long long n = rows * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long row = i / C;
        const int c = (int)(i - row * C);
        const unsigned short* line = reinterpret_cast<const unsigned short*>(x) + row * C * 2 + (c >> 5) * 64 + (c & 31);
        out[i] = __builtin_bit_cast(float, (unsigned)line[0] << 16) + __builtin_bit_cast(float, (unsigned)line[32] << 16);
    }
}

}  // namespace

void launch_split32_unpack(const Ctx& ctx, const float* x, long long rows, int C, float* out) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 32 == 0, "split32 rows are whole 32-channel lines");
    const long long n = rows * C;
    const unsigned grid = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    hipLaunchKernelGGL(split32_unpack_kernel, dim3(grid), dim3(256), 0, ctx.stream, x, rows, C, out);
    MAA_HIP(hipGetLastError());
}

void launch_split32_pack(const Ctx& ctx, const float* x, long long rows, int C, float* out, float slope) {
    if (ctx.ws.dry) return;
    ProfScope prof(ctx, "split32_pack_kernel", 0.0, 8.0 * rows * (double)C);
    MAA_CHECK(C % 32 == 0, "split32 rows are whole 32-channel lines");
    const long long n4 = rows * (C / 4);
    const unsigned grid = (unsigned)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256);
    hipLaunchKernelGGL(split32_pack_kernel, dim3(grid), dim3(256), 0, ctx.stream, x, rows, C, slope, out);
    MAA_HIP(hipGetLastError());
}

void launch_groupnorm(Ctx& ctx, const float* x1, int ld1, int C1, const float* x2, int ld2, int C2, int B, int HW,
                      int groups, const float* gamma, const float* beta, float eps, int silu, float* out,
                      int out_split, float* raw_split) {
    const int C = C1 + C2;
    float* tab = ctx.ws.alloc_f((size_t)2 * B * C);    // per-(sample, channel) {scale, shift}; released with the caller's arena mark
    if (ctx.ws.dry) return;
    MAA_CHECK(C % groups == 0 && C / groups <= 256 && C % 4 == 0 && C1 % 4 == 0 && ld1 % 4 == 0 && (C2 == 0 || ld2 % 4 == 0),
              "groupnorm channels");
    ProfScope prof(ctx, "groupnorm", 0.0, 8.0 * B * (double)HW * C);
    const GnFusedPlan fp = ctx.tune.gn_two_pass ? GnFusedPlan() : gn_fused_plan(C, C1, HW, groups);
    if (fp.gpb) {
        const int nblk = groups / fp.gpb;
        dim3 grid((unsigned)(nblk * B));
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, grid, dim3((unsigned)fp.threads), fp.lds, ctx.stream, x1, ld1, C1, x2, ld2, C2, HW, groups, fp.gpb, eps,
                               gamma, beta, silu, out, out_split, raw_split, nblk);
        };
        switch (fp.nr) {
            case 1: go(gn_fused_kernel<1>); break;
            case 2: go(gn_fused_kernel<2>); break;
            case 4: go(gn_fused_kernel<4>); break;
            case 8: go(gn_fused_kernel<8>); break;
            case 12: go(gn_fused_kernel<12>); break;
            default: go(gn_fused_kernel<16>); break;
        }
        MAA_HIP(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL(gn_stats_kernel, dim3(B * groups), dim3(256), 0, ctx.stream, x1, ld1, C1, x2, ld2, C2, HW, groups,
                       eps, gamma, beta, tab);
    const int rb = (HW + 15) / 16, passes = (C / 4 + 15) / 16;
    int nz = (768 + rb * B - 1) / (rb * B);         // aim at >= 3 workgroups per CU
    nz = nz < 1 ? 1 : nz > passes ? passes : nz;
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)rb, (unsigned)B, (unsigned)nz), dim3(256), 0, ctx.stream, x1, ld1,
                       C1, x2, ld2, C2, HW, tab, silu, out, out_split, raw_split);
    MAA_HIP(hipGetLastError());
}

void launch_layernorm(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta,
                      float eps, float* out, int out_split) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C <= 2048 && C % 4 == 0, "layernorm width");
    ProfScope prof(ctx, "layernorm", 0.0, 8.0 * rows * (double)C);
    const dim3 grid = row_grid(rows);
    if (C <= 256)
        hipLaunchKernelGGL(layernorm_kernel<1>, grid, dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, out, out_split);
    else if (C <= 512)
        hipLaunchKernelGGL(layernorm_kernel<2>, grid, dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, out, out_split);
    else if (C <= 1024)
        hipLaunchKernelGGL(layernorm_kernel<4>, grid, dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, out, out_split);
    else      // the ViT-H image tower's 1280-wide rows
        hipLaunchKernelGGL(layernorm_kernel<8>, grid, dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, out, out_split);
    MAA_HIP(hipGetLastError());
}

void launch_softmax(const Ctx& ctx, float* s, long long rows, int cols, int ld, int causal_nq) {
    if (ctx.ws.dry) return;
    MAA_CHECK(ld >= cols, "softmax ld");
    ProfScope prof(ctx, "softmax", 0.0, 8.0 * rows * (double)ld);
    const dim3 grid = row_grid(rows);
    if (ld <= 128)
        hipLaunchKernelGGL(softmax_kernel<2>, grid, dim3(256), 0, ctx.stream, s, rows, cols, ld, causal_nq);
    else if (ld <= 256)
        hipLaunchKernelGGL(softmax_kernel<4>, grid, dim3(256), 0, ctx.stream, s, rows, cols, ld, causal_nq);
    else if (ld <= 1088)
        hipLaunchKernelGGL(softmax_kernel<17>, grid, dim3(256), 0, ctx.stream, s, rows, cols, ld, causal_nq);
    else
        hipLaunchKernelGGL(softmax_kernel<0>, grid, dim3(256), 0, ctx.stream, s, rows, cols, ld, causal_nq);
    MAA_HIP(hipGetLastError());
}

void launch_softmax_masked(const Ctx& ctx, float* s, long long rows, int cols, int ld, const float* key_mask, long long rows_per_sample) {
    if (ctx.ws.dry) return;
    MAA_CHECK(ld >= cols && key_mask && rows_per_sample > 0, "masked softmax arguments");
    ProfScope prof(ctx, "softmax", 0.0, 8.0 * rows * (double)ld);
    hipLaunchKernelGGL(softmax_masked_kernel, row_grid(rows), dim3(256), 0, ctx.stream, s, rows, cols, ld, key_mask,
                       rows_per_sample);
    MAA_HIP(hipGetLastError());
}

}  // namespace maa
