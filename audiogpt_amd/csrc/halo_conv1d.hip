// Dilated "same" Conv1d for the narrow stages of the HiFi-GAN / BigVGAN MRF resblocks (C = 32 or 64 channels in and out),
// bf16x3 arithmetic: the input tile is staged ONCE in LDS and every tap reads it at a row offset.
//
// Replaces, at those widths, Conv1d(C, C, k, dilation = d, padding = (k d - d) / 2) with its preceding leaky-ReLU inside
// ResBlock1 (NeuralSeq/modules/hifigan/hifigan.py:30-67) and the convs of AMPBlock1 (vocoder/bigvgan/models.py:30-81).
//
// Why.  At 22.05 kHz config-3 scale these layers are [64 x 262144, 32] and [64 x 131072, 64] tensors: 2.1 GB each way.  As a
// generic implicit GEMM a workgroup fetches its 256 x 32-channel A rows again for each of the k taps (k = 3, 7, 11): 36 KB
// through the texture path per 384 MFMA cycles = 96 B/clk/CU, above what that path moves (~64 B/clk/CU), so the layer runs
// at 48 TFLOP/s (1.3 TB/s of HBM-side bytes) -- bound by L1/L2 re-reads, not by HBM and not by the MFMAs.  Per output
// element the layer needs 2 k C multiply-adds (192 .. 1408 flops at C = 32 / 64) against 12 bytes of HBM (input, residual,
// output): at 8 TB/s the HBM bound is 16x (C = 32, k = 3) .. 1.1x (C = 64, k = 11) below the bf16x3 MFMA bound, i.e. the
// layer should be HBM-bound.  Staging the tile once makes the L2->CU bytes equal to the HBM bytes.
//
// One workgroup (4 waves) per tile of TL = 256 (C = 32) or 128 (C = 64) rows of one sample; persistent over tiles.  HaloTile
// holds what the two kernels of this file are made of:
//   * stage_image -- A image: rows pos0 .. pos0 + rows - 1 (tile + halo, H = d (k-1) / 2 <= HMAX each side) read as fp32
//     (coalesced float4 x 2 per lane), leaky-ReLU applied, split into bf16 hi / lo and written as split32 lines
//     (ds_write_b128, slot XOR-swizzled by (row >> 1) & 7); rows outside [0, L) are zeros (the conv's zero padding; leaky(0) = 0)
//   * start / issue -- B: the packed split32 weights [C][k C] stream through an NSB-stage LDS ring by LDS-DMA, chunk c =
//     (tap, 32-channel block); the chunks of up to two weight tensors follow each other in ONE sequence
//   * conv_chunks -- wave w owns rows 32 MI w .. (two 32-row MFMA blocks at TL = 256) x all C outputs; for chunk (tap t, block
//     cb) its A fragments are rows i + t d of line cb of the image -- no data moves, only the row index.  Products per
//     accumulator: lo.hi, hi.lo, hi.hi per 16-deep k-step (mma_kstep), K ordered (tap, channel) -- exactly the generic
//     engines' arithmetic, so results are bit-identical to them (tests)
//   * epilogue -- shared with the implicit-GEMM engines (bias, residual, out_scale, accumulate), rows past the tile masked
// halo_conv1d_kernel: stage, chunks [0, n), epilogue.  halo_pair_kernel (the fused MRF pair, below): stage, chunks [0, n1),
// the intermediate image, chunks [n1, n), epilogue.
#include "igemm_epilogue.h"

namespace maa {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int HMAX = 32;           // halo rows reserved on each side (needs d (k-1) / 2 <= HMAX)
constexpr int HMAX2 = 16;          // rows the pair's second convolution may reach past the t image (d2 (k2 - 1) <= HMAX2)

// The thread index is read where it is used, never kept in HaloTile: out of a struct member the compiler no longer knows its
// range, and the staging then holds 8 - 10 VGPRs of addresses it does not fold.  (wid / lrow / lk ARE members, computed once in
// init: a readfirstlane per issue() is one per chunk and cost the one-convolution kernel 1 - 3 %.)
__device__ __forceinline__ int thread_id() { return threadIdx.x; }

// TL = rows per tile (4 waves x MI 32-row blocks); NSB = weight ring stages
template <int C, int TL, int NSB>
struct HaloTile {
    static_assert(TL == 128 || TL == 256, "tile length");
    static constexpr int AROWS = TL + 2 * HMAX;
    static constexpr int CB = C / 32;                 // 128-byte lines per row = 32-channel blocks
    static constexpr int NI = C / 32, MI = TL / 128;
    static constexpr int A_BYTES = AROWS * CB * 128;
    static constexpr int BSTAGE = C * 128;            // one weight chunk: C rows x 128 B
    static constexpr int IPW = C / 32;                // LDS-DMA copies (8 rows x 128 B) per wave and chunk: C / 8 / 4 waves
    static constexpr int LDS_BYTES = A_BYTES + NSB * BSTAGE;
    static_assert(LDS_BYTES <= 163840, "LDS per workgroup");
    static_assert(TL + HMAX2 <= AROWS, "the pair's t image inside the x image");

    char* smem;                    // [AROWS][CB][128] image | [NSB][C][128] weight ring
    int wid, lrow, lk;             // wave; row / column inside a 32-wide MFMA block; half of a 16-deep k-step
    const char *wrow1[IPW], *wrow2[IPW], *zeros;
    int n1, nchunks;               // chunks [0, n1) come from the first weight tensor, [n1, nchunks) from the second
    int st, st_fill;               // ring stage of the next chunk to multiply / to refill
    int b_off[2][2];               // B fragment offsets inside a stage (rows n = j 32 + lrow)

    // One weight tensor: n2 = 0.  Weight copies: copy q covers weight rows 8q .. 8q+7; this wave issues q = j 4 + wid (j < IPW)
    __device__ __forceinline__ void init(const float* w1, int ldb1, int n1_, const float* w2, int ldb2, int n2, const float* z) {
        extern __shared__ __attribute__((aligned(1024))) char lds[];
        smem = lds;
        const int lane = thread_id() & 63;
        wid = __builtin_amdgcn_readfirstlane(thread_id() >> 6);
        lrow = lane & 31, lk = lane >> 5;
        n1 = n1_, nchunks = n1_ + n2;
        zeros = reinterpret_cast<const char*>(z);
        const int r8 = lane >> 3;
        const int bslot = (((lane & 7) ^ (((wid & 1) << 2) + (r8 >> 1))) << 4);
#pragma unroll
        for (int j = 0; j < IPW; ++j) {
            wrow1[j] = reinterpret_cast<const char*>(w1) + (long long)(8 * (j * 4 + wid) + r8) * ldb1 * 4 + bslot;
            wrow2[j] = reinterpret_cast<const char*>(w2) + (long long)(8 * (j * 4 + wid) + r8) * ldb2 * 4 + bslot;
        }
        frag_slot_offsets(lrow, lk, b_off);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) b_off[pl][ks] += lrow * 128;
    }

    __device__ __forceinline__ void issue(int stage, int chunk) const {
        const bool live = chunk < nchunks, first = chunk < n1;
#pragma unroll
        for (int j = 0; j < IPW; ++j) {
            const char* src = !live ? zeros : first ? wrow1[j] + (long long)chunk * 128 : wrow2[j] + (long long)(chunk - n1) * 128;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + A_BYTES + stage * BSTAGE + (j * 4 + wid) * 1024), 16, 0, 0);
        }
    }

    // A tile begins: the weights of the first chunks go out first, their latency hides behind the A staging
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int s = 0; s < NSB - 1; ++s) issue(s, s);
        st = 0, st_fill = NSB - 1;
    }

    // A image of leaky(x): image row r <-> position pos0 + r of the sample x, r < rows; 8 channels (32 B fp32 -> 16 B hi +
    // 16 B lo) per piece.  All of a thread's loads go out before the first conversion (addresses clamped into the sample,
    // values masked afterwards), so a tile pays one memory latency, not one per piece.
    __device__ __forceinline__ void stage_image(const float* x, int pos0, int rows, int L, float slope) const {
        constexpr int PPR = C / 8;                      // pieces per row
        constexpr int NPT = (AROWS * PPR + 255) / 256;  // pieces per thread (upper bound)
        const int tid = thread_id();
        float4 v0[NPT], v1[NPT];
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
            const int p0 = tid + 256 * u;
            const int r = p0 / PPR, q = p0 - r * PPR;
            int l = pos0 + r;
            l = l < 0 ? 0 : (l >= L ? L - 1 : l);
            const float4* src = reinterpret_cast<const float4*>(x + (long long)l * C + q * 8);
            v0[u] = src[0];
            v1[u] = src[1];
        }
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
            const int p0 = tid + 256 * u;
            const int r = p0 / PPR, q = p0 - r * PPR;
            const int l = pos0 + r;
            if (r < rows) {
                const float s = (l >= 0 && l < L) ? slope : 0.f;      // rows outside the sample: zeros (x * 0, then max(0, 0))
                const float m = (l >= 0 && l < L) ? 1.f : 0.f;
                float4 w0 = v0[u], w1 = v1[u];
                w0.x = fmaxf(w0.x * m, w0.x * s);
                w0.y = fmaxf(w0.y * m, w0.y * s);
                w0.z = fmaxf(w0.z * m, w0.z * s);
                w0.w = fmaxf(w0.w * m, w0.w * s);
                w1.x = fmaxf(w1.x * m, w1.x * s);
                w1.y = fmaxf(w1.y * m, w1.y * s);
                w1.z = fmaxf(w1.z * m, w1.z * s);
                w1.w = fmaxf(w1.w * m, w1.w * s);
                unsigned h0, h1, h2, h3, q0, q1, q2, q3;
                split2(w0.x, w0.y, h0, q0);
                split2(w0.z, w0.w, h1, q1);
                split2(w1.x, w1.y, h2, q2);
                split2(w1.z, w1.w, h3, q3);
                const u32x4 hi = {h0, h1, h2, h3}, lo = {q0, q1, q2, q3};
                // channels 8q .. 8q+7 of line cb = q / 4: hi slot (q & 3), lo slot 4 + (q & 3), swizzled by the row
                const int cb = q >> 2, sl = q & 3, sw = (r >> 1) & 7;
                char* line = smem + (r * CB + cb) * 128;
                *reinterpret_cast<u32x4*>(line + ((sl ^ sw) << 4)) = hi;
                *reinterpret_cast<u32x4*>(line + (((4 + sl) ^ sw) << 4)) = lo;
            }
        }
        wait_lgkm0();
    }

    // Chunks [c_begin, c_end) of the weight sequence = one convolution with dilation dil out of the image, taps ascending.
    // The ring does not restart between two convolutions of a tile: c counts on.
    __device__ __forceinline__ void conv_chunks(f32x16 (&acc)[MI][NI], int c_begin, int c_end, int dil) {
        int tap = 0, cb = 0;
        for (int c = c_begin; c < c_end; ++c) {
            wait_vmcnt<(NSB - 2) * IPW>();
            __builtin_amdgcn_s_barrier();          // chunk c of the weights is in LDS (and, at c = c_begin, the whole image)
            issue(st_fill, c + NSB - 1);
            const char* bst = smem + A_BYTES + st * BSTAGE;
            bf16x8 ah[2][MI], al[2][MI], bh[2][NI], bl[2][NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int row = wid * (32 * MI) + i * 32 + lrow + tap * dil;      // image row of this lane's output row + tap
                const char* line = smem + (row * CB + cb) * 128;
                const int sw = (row >> 1) & 7;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    ah[ks][i] = *reinterpret_cast<const bf16x8*>(line + (((ks * 2 + lk) ^ sw) << 4));
                    al[ks][i] = *reinterpret_cast<const bf16x8*>(line + (((4 + ks * 2 + lk) ^ sw) << 4));
                }
            }
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    bh[ks][j] = *reinterpret_cast<const bf16x8*>(bst + j * 4096 + b_off[0][ks]);
                    bl[ks][j] = *reinterpret_cast<const bf16x8*>(bst + j * 4096 + b_off[1][ks]);
                }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) mma_kstep<3, MI, NI>(acc, ah[ks], al[ks], bh[ks], bl[ks]);
            st = st + 1 == NSB ? 0 : st + 1;
            st_fill = st_fill + 1 == NSB ? 0 : st_fill + 1;
            if (++cb == CB) {
                cb = 0;
                ++tap;
            }
        }
    }

    // Output rows 0 .. tlo - 1 of the tile <-> positions l0 .. of sample b; rows of the next tile / past the sample are masked by M
    __device__ __forceinline__ void epilogue(const IGemm& g, f32x16 (&acc)[MI][NI], int b, int L, int l0, int tlo) const {
        wait_vmcnt<0>();                           // (the trailing copies were dummies)
        IGemm q = g;
        const int mrow0 = b * L + l0;
        q.M = b * L + min(L, l0 + tlo);
        igemm_epilogue<MI, NI>(q, acc, mrow0 + wid * (32 * MI), 0, lrow, lk, 0, C, 1);
        __builtin_amdgcn_s_barrier();              // everybody is done reading the image before the next tile overwrites it
    }
};

struct HaloArgs {
    IGemm g;            // epilogue fields (bias, res, ldr, out_scale, accumulate, c, ldc, N, alpha), b / ldb (weights), zeros
    const float* x;     // [B, L, C] fp32
    int B, L, k, dil;
    float slope;        // leaky-ReLU slope of the prologue (1 = none)
    int tiles_per_sample, tiles;
};

template <int C, int TL, int NSB>
__global__ __launch_bounds__(256) void halo_conv1d_kernel(const HaloArgs a) {
    using T = HaloTile<C, TL, NSB>;
    const int H = a.dil * (a.k - 1) / 2;
    const int nchunks = a.k * T::CB;
    T t;
    t.init(a.g.b, a.g.ldb, nchunks, a.g.b, a.g.ldb, 0, a.g.zeros);
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int b = tile / a.tiles_per_sample;
        const int l0 = (tile - b * a.tiles_per_sample) * TL;
        t.start();
        t.stage_image(a.x + (long long)b * a.L * C, l0 - H, TL + 2 * H, a.L, a.slope);
        f32x16 acc[T::MI][T::NI];
        zero_acc(acc);
        t.conv_chunks(acc, 0, nchunks, a.dil);
        t.epilogue(a.g, acc, b, a.L, l0, TL);
    }
}

// ---------------------------------------------------------------------------------------------------------------- fused MRF pair
// One launch for the pair of an MRF resblock at the narrow stages (hifigan.py:54-61):
//     xt = c1(leaky(x));  xt = c2(leaky(xt));  x' = xt + x          (c1: k taps, dilation d1;  c2: k taps, dilation d2 = 1)
// The intermediate tensor never leaves the CU: 20 B of HBM traffic per element and pair (x in, t out, t in, x as residual, x' out)
// become 8 + the residual's re-read out of L2, and there is one staging pass and one launch instead of two.
//
// What differs from the one-convolution kernel.  A tile is R1 = TL rows of t -- positions t0 = l0 - H2 .. t0 + R1 - 1, H2 =
// d2 (k2 - 1) / 2 -- out of the image of leaky(x) staged from row t0 - H1.  Between the convolutions the accumulators take the
// first epilogue in registers (+ bias1, rows outside the sample -> 0: c2's zero padding), leaky-ReLU, hi / lo split, and are
// written over the x image as the split32 image of leaky(t) (the accumulator layout holds one column per lane: lane pairs swap
// halves so that every lane writes whole 4-byte words).  Of the second convolution's R1 output rows the first TLo = R1 - 2 H2
// are positions l0 .. l0 + TLo - 1 and are stored; the last 2 H2 rows multiply rows past the image and are dropped.
// Arithmetic = the two launches': same products, same order (the same HaloTile code), same fp32 epilogue in between --
// bit-identical (tests).
struct HaloPairArgs {
    IGemm g;             // second convolution: b / ldb / bias, res, ldr, out_scale, accumulate, c, ldc, N, zeros
    const float* x;      // [B, L, C] fp32
    const float* w1;     // first convolution: packed split32 weights [C][k1 C], pitch ldb1 floats
    const float* bias1;
    int ldb1;
    int B, L, k1, d1, k2, d2;
    float slope1, slope2;
    int TLo, tiles_per_sample, tiles;
};

template <int C, int TL, int NSB>
__global__ __launch_bounds__(256) void halo_pair_kernel(const HaloPairArgs a) {
    using T = HaloTile<C, TL, NSB>;
    constexpr int CB = T::CB, MI = T::MI, NI = T::NI;
    const int H1 = a.d1 * (a.k1 - 1) / 2, H2 = a.d2 * (a.k2 - 1) / 2;
    const int n1 = a.k1 * CB, n2 = a.k2 * CB;
    const int tid = thread_id();
    T t;
    t.init(a.w1, a.ldb1, n1, a.g.b, a.g.ldb, n2, a.g.zeros);
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int b = tile / a.tiles_per_sample;
        const int l0 = (tile - b * a.tiles_per_sample) * a.TLo;
        const int t0 = l0 - H2;                    // position of row 0 of the t image
        t.start();
        t.stage_image(a.x + (long long)b * a.L * C, t0 - H1, TL + 2 * H1, a.L, a.slope1);
        f32x16 acc[MI][NI];
        zero_acc(acc);
        t.conv_chunks(acc, 0, n1, a.d1);
        // ---- between the convolutions: t = acc + bias1 (the first launch's epilogue), rows outside the sample are c2's
        // zero padding, leaky-ReLU and split exactly as the second launch's staging did, written over the x image
        __builtin_amdgcn_s_barrier();              // every wave has read its last x rows
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int n = j * 32 + t.lrow;
                const float bv = a.bias1 ? a.bias1[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = t.wid * (32 * MI) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * t.lk;
                    const int l = t0 + row;
                    const bool in = l >= 0 && l < a.L;
                    float v = acc[i][j][r] * 1.0f + bv;
                    v = in ? fmaxf(v * 1.f, v * a.slope2) : 0.f;
                    // lanes 2m / 2m + 1 hold columns n / n + 1 of the same row: the even lane writes both hi halves, the odd
                    // lane both lo halves (one 4-byte LDS store per lane and element)
                    const bool even = (tid & 1) == 0;
                    // channel pair (n & ~1) of line j: 16-byte slot ((n & 31) >> 3) (+ 4 for the lo half), swizzled by the row
                    const int sl = ((n & 31) >> 3) + (even ? 0 : 4), sw = (row >> 1) & 7;
                    char* line = t.smem + (row * CB + j) * 128;
                    *reinterpret_cast<unsigned*>(line + ((sl ^ sw) << 4) + ((n & 6) << 1)) = split_pair_word(even, v);
                }
            }
        // rows TL .. TL + 2 H2 - 1 of the t image feed only output rows that are dropped, but must be finite
        for (int e = tid; e < 2 * H2 * CB * 8; e += 256)
            reinterpret_cast<u32x4*>(t.smem + TL * CB * 128)[e] = u32x4{0u, 0u, 0u, 0u};
        zero_acc(acc);
        wait_lgkm0();
        t.conv_chunks(acc, n1, n1 + n2, a.d2);
        t.epilogue(a.g, acc, b, a.L, l0, a.TLo);
    }
}

// Persistent grid: as many workgroups as fit the CUs by LDS (at most 3 per CU), no more than tiles
template <int C, int TL, int NSB, class Args>
void launch_tiles(const Ctx& ctx, void (*kern)(const Args), const Args& a) {
    constexpr size_t lds = HaloTile<C, TL, NSB>::LDS_BYTES;
    ensure_dynamic_lds(reinterpret_cast<const void*>(kern), ctx.device, (int)lds);
    const int nc = device_cu_count(ctx.device);
    const int per_cu = (int)(163840 / lds) < 3 ? (int)(163840 / lds) : 3;
    long long grid = (long long)nc * (per_cu < 1 ? 1 : per_cu);
    if (grid > a.tiles) grid = a.tiles;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, ctx.stream, a);
}

// One convolution the kernels cover: bf16x3 mode, C = 32 / 64 in and out, split32 weights packed [C][k C], odd k, "same"
// padding reaching d (k - 1) <= reach rows over both sides; x 16-byte aligned and indexable with 31 bits.
// (C = 128 was tried with a 128-position tile, one workgroup per CU: 72.3 ms vs 70.6 ms for the generic engine on the
//  config-3 stage -- at that width the layer is MFMA-bound and gains nothing from the staging; not kept)
bool halo_covers(const Ctx& ctx, const float* x, int B, int L, int C, const PackedW& w, int k, int dil, int reach) {
    if (ctx.dtype != 1 || !(C == 32 || C == 64) || w.N != C || w.K != k * C || !w.split || !w.nk) return false;
    if (k < 1 || (k & 1) == 0 || dil < 1 || dil * (k - 1) > reach) return false;
    return (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (long long)B * L * C < (1ll << 31);
}

// The epilogue of a launch, as conv_into: bias and weights of the (last) convolution, residual, out_scale, accumulate
void fill_epilogue(IGemm& g, const Ctx& ctx, const PackedW& w, int B, int L, int C, const float* res, float out_scale,
                   int accumulate, float* out) {
    g.b = w.w;
    g.ldb = w.ld;
    g.bias = w.bias;
    g.res = res;
    g.ldr = C;
    g.out_scale = out_scale;
    g.accumulate = accumulate;
    g.c = out;
    g.ldc = C;
    g.N = C;
    g.M = B * L;
    g.zeros = ctx.zeros;
}

}  // namespace

// Conv1d(C, C, k, dilation) with "same" padding on x [B, L, C] (fp32, channels-last), optional leaky-ReLU prologue, epilogue
// as conv_into (bias from the packed weight, residual, out_scale, accumulate).  false: shape / mode not covered -- the caller
// uses the generic implicit GEMM.  MAA_HALO=off disables it (A/B, bit-identity tests).
bool launch_halo_conv1d(const Ctx& ctx, const float* x, int B, int L, int C, const PackedW& w, int k, int dil, float slope,
                        const float* res, float out_scale, int accumulate, float* out) {
    if (ctx.tune.halo == 0 || !halo_covers(ctx, x, B, L, C, w, k, dil, 2 * HMAX)) return false;
    if (ctx.ws.dry) return true;
    HaloArgs a;
    fill_epilogue(a.g, ctx, w, B, L, C, res, out_scale, accumulate, out);
    a.x = x;
    a.B = B;
    a.L = L;
    a.k = k;
    a.dil = dil;
    a.slope = slope;
    // tile length: 256 positions at C = 32 (56 KB of LDS, two workgroups per CU); 128 at C = 64 (80 KB: still two per CU, so
    // one workgroup's tile staging overlaps the other's MFMAs; 256 would be 112 KB and one per CU, and measured slower:
    // profiles/r2_halo_conv1d_variants.txt)
    const int TLr = C == 32 ? 256 : 128;
    a.tiles_per_sample = (L + TLr - 1) / TLr;
    a.tiles = B * a.tiles_per_sample;
    const double flops = 2.0 * B * (double)L * C * (double)C * k;
    ProfScope prof(ctx, C == 32 ? "halo_conv1d_bf16x3<32>" : "halo_conv1d_bf16x3<64>", flops, 12.0 * B * (double)L * C);
    if (C == 32)
        launch_tiles<32, 256, 4>(ctx, halo_conv1d_kernel<32, 256, 4>, a);
    else
        launch_tiles<64, 128, 4>(ctx, halo_conv1d_kernel<64, 128, 4>, a);
    MAA_HIP(hipGetLastError());
    return true;
}

// The MRF pair x' = (c2(leaky(c1(leaky(x)))) + res) * out_scale (+ out) in one launch; conditions as launch_halo_conv1d for both
// convolutions (same C, odd kernels, "same" padding), d2 (k2 - 1) <= HMAX2.  false: not covered -- the caller launches the two
// convolutions.  MAA_HALO=single (or off) disables it (A/B, bit-identity tests).
bool launch_halo_pair(const Ctx& ctx, const float* x, int B, int L, int C, const PackedW& w1, int k1, int d1, float slope1,
                      const PackedW& w2, int k2, int d2, float slope2, const float* res, float out_scale, int accumulate,
                      float* out) {
    if (ctx.tune.halo != 2 || !halo_covers(ctx, x, B, L, C, w1, k1, d1, 2 * HMAX) || !halo_covers(ctx, x, B, L, C, w2, k2, d2, HMAX2))
        return false;
    if (ctx.ws.dry) return true;
    HaloPairArgs a;
    fill_epilogue(a.g, ctx, w2, B, L, C, res, out_scale, accumulate, out);
    a.x = x;
    a.w1 = w1.w;
    a.bias1 = w1.bias;
    a.ldb1 = w1.ld;
    a.B = B;
    a.L = L;
    a.k1 = k1;
    a.d1 = d1;
    a.k2 = k2;
    a.d2 = d2;
    a.slope1 = slope1;
    a.slope2 = slope2;
    const int TLr = C == 32 ? 256 : 128;
    a.TLo = TLr - d2 * (k2 - 1);
    a.tiles_per_sample = (L + a.TLo - 1) / a.TLo;
    a.tiles = B * a.tiles_per_sample;
    const double flops = 2.0 * B * (double)L * C * (double)C * (k1 + k2);
    ProfScope prof(ctx, C == 32 ? "halo_pair_bf16x3<32>" : "halo_pair_bf16x3<64>", flops, 12.0 * B * (double)L * C);
    if (C == 32)
        launch_tiles<32, 256, 4>(ctx, halo_pair_kernel<32, 256, 4>, a);
    else
        launch_tiles<64, 128, 4>(ctx, halo_pair_kernel<64, 128, 4>, a);
    MAA_HIP(hipGetLastError());
    return true;
}

}  // namespace maa
