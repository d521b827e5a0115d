// Implicit-GEMM engine on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, gfx950), fp32 in / fp32 out.
//
// Same problem description (IGemm), gather and epilogue as igemm_f32.hip; what changes is how the fp32 operands
// reach the MFMA:
//   TERMS = 3  "bf16x3": every fp32 operand is split on the fly into hi = bf16(x) and lo = bf16(x - hi) while its
//              tile is written to LDS, and the product is formed as lo*hi + hi*lo + hi*hi with fp32 accumulation.
//              hi+lo carries 16 mantissa bits, so a product is good to ~2^-16 instead of bf16's 2^-8, at 3 MFMAs
//              per 16-deep k-step: 16/3 = 5.3x the fp32 MFMA rate (gfx950 has no TF32/xf32, and its fp32 MFMA runs
//              at 1/16 of the bf16 rate, so this is the fast path that still meets the fp32 parity gates).
//   TERMS = 1  plain bf16 operands (throughput mode; error reported, not gated at 1e-4).
// LDS tiles are row-major with k contiguous: [row][32 k] bf16 = 64-byte rows, no padding, one plane for hi and one
// for lo; the four 16-byte slots of a row are XOR-swizzled by (row >> 2) & 3, so a lane's MFMA operand (8 consecutive
// k of one row) is one conflict-free ds_read_b128.  B must be given k-contiguous ([N][K]: packed weights in this
// mode, and K of Q.K^T).
// This is the REGISTER-STAGED engine (global -> VGPR -> LDS): it takes fp32 operands (split on the fly while the tile
// is written to LDS) and split32 operands alike.  Problems whose operands are BOTH split32 go to the LDS-DMA engine
// (igemm_dma.hip) in the bf16x3 mode; the two engines issue the same products in the same order.
#include "igemm_epilogue.h"

#include <cstdlib>

namespace maa {

namespace {

constexpr int NT = 256;

// A_SPLIT / B_SPLIT: the operand already sits in memory pre-split ("split32" format: each group of 32 consecutive k
// of a row occupies one 128-byte line = [32 bf16 hi | 32 bf16 lo], so a row has the byte pitch of its fp32 form):
// GroupNorm / LayerNorm outputs and packed weights in the bf16 modes.  A tile row of one K chunk is then exactly one
// cache line, fetched once, and is copied global -> LDS as 16-byte pieces with no conversion.  Otherwise the operand
// is fp32 and is split while its tile is written to LDS (once per tile, i.e. once per tap and per N-tile for a
// conv -- which is why producers pre-split).
__device__ __forceinline__ void st16(unsigned short* dst, const float4& v) {   // 16-byte LDS store, by members
    const f32x4 t = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<f32x4*>(dst) = t;
}

// BK: K depth of one LDS stage (32).  PF: register prefetch depth in K chunks (even).  The tile loads of chunk c + PF
// are issued before the MFMAs of chunk c and are first needed PF chunk-times later, when they are copied to LDS.
// Most of them miss L2 on first touch (a conv's weights alone are 3-4x one XCD's L2, and every XCD streams all of
// them), so a load takes ~2000 cycles: with PF = 2 a 64x64 chunk could not go faster than ~1000 cycles -- five times
// its MFMA time.  vmcnt retires in order, so only more register sets (or more waves) put more bytes in flight.
template <int BM, int BN, int WGM, int WGN, int TERMS, bool A_SPLIT, bool B_SPLIT, int BK, int PF>
__global__ __launch_bounds__(NT) void igemm_bf16_kernel(const IGemm p, int ntiles, int Nb) {
    // LDS rows are 64 B (32 bf16) with NO padding; the 16-byte chunk c of row r is stored at chunk c ^ ((r >> 2) & 3).
    // That XOR swizzle makes both the ds_write_b128 of the staging pass (8-lane groups = two rows = 32 distinct
    // banks) and the ds_read_b128 of the MFMA operands (16-lane groups {0-3,12-15,20-27} -> 16 distinct 16-byte
    // slots) conflict-free, and saves the 25 % of LDS a padded pitch costs.
    static_assert(BK == 32, "swizzle is written for 4 chunks per row");
    constexpr int LDK = BK;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int MI = WTM / 32, NI = WTN / 32;
    constexpr int PLANES = TERMS == 1 ? 1 : 2;
    constexpr int ROWS = BM + BN;
    constexpr int PLANE_ELEMS = ROWS * LDK;            // bf16 elements of one plane of one buffer
    // per-thread 16-byte loads per chunk: fp32 operand: rows/32 float4; split operand: (rows/64 row slots) x planes
    // both operand forms: 8 threads per row, 16 bytes each = the 128-byte line of one (row, K chunk); 32 rows per pass
    constexpr int RPP = NT / 8;
    constexpr int ARS = BM / RPP, BRS = BN / RPP;     // row slots (= 16-byte loads) per thread per chunk
    constexpr int AL = ARS, BL = BRS;
    static_assert(WGM * WGN == 4 && BM % 32 == 0 && BN % 32 == 0, "tile");
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];   // [buf][plane][row][LDK]

    const int tid = threadIdx.x;
    const int bid = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);      // consecutive tiles (N-tiles fastest) on one XCD: igemm_device.h
    const int nt = bid % ntiles, mt = bid / ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int z = blockIdx.y;
    const int zo = z / p.zin, zi = z - zo * p.zin;
    const float* a1 = p.a1 + zo * p.a_so + zi * p.a_si;
    const float* a2 = p.a2;
    const float* bp = p.b + zo * p.b_so + zi * p.b_si;
    const long long coff = zo * p.c_so + zi * p.c_si;

    const int Ctot = p.C1 + p.C2;
    const int rpb = p.Hout * p.Wout;
    const int Hlim = p.Hin << p.up, Wlim = p.Win << p.up;
    const int taps = p.KH * p.KW;
    const float4* g_zero4 = reinterpret_cast<const float4*>(p.zeros);
    const float slope = p.a_act == 1 ? p.a_slope : 1.0f;

    // thread -> (row slot, k offset) for each operand form
    const int a_r0 = tid >> 3, b_r0 = tid >> 3;
    constexpr int a_rstep = RPP, b_rstep = RPP;
    const int seg = tid & 7;                 // 16-byte piece of the line: fp32 -> k = 4 seg; split32 -> plane seg>>2, chunk seg&3
    const int a_k = seg * 4, b_k = seg * 4;  // offset in fp32 units (4 bytes) for both forms

    // ---- A rows of this thread
    int a_b[ARS], a_iy0[ARS], a_ix0[ARS];
#pragma unroll
    for (int j = 0; j < ARS; ++j) {
        const int row = a_r0 + a_rstep * j;
        const int m = m0 + row;
        if (row < BM && m < p.M) {
            const int b = m / rpb;
            const int rem = m - b * rpb;
            const int oy = rem / p.Wout;
            const int ox = rem - oy * p.Wout;
            a_b[j] = b;
            a_iy0[j] = oy * p.sh - p.ph;
            a_ix0[j] = ox * p.sw - p.pw;
        } else {
            a_b[j] = -1;
            a_iy0[j] = 0;
            a_ix0[j] = 0;
        }
    }
    const void* a_p1[ARS];
    const void* a_p2[ARS];
    bool a_ok[ARS];
    int g_tap = 0, g_ci = 0;
    auto set_tap = [&](int tap) {
        const int ky = tap / p.KW, kx = tap - ky * p.KW;
#pragma unroll
        for (int j = 0; j < ARS; ++j) {
            int iy = a_iy0[j] + ky * p.dh, ix = a_ix0[j] + kx * p.dw;
            const bool ok = a_b[j] >= 0 && iy >= 0 && iy < Hlim && ix >= 0 && ix < Wlim;
            iy >>= p.up;
            ix >>= p.up;
            const long long off = ok ? ((long long)a_b[j] * p.Hin + iy) * p.Win + ix : 0;
            a_ok[j] = ok;
            a_p1[j] = a1 + off * p.lda1 + a_k;
            a_p2[j] = a2 + off * p.lda2 + a_k - p.C1;
        }
    };
    auto load_a = [&](float4 (&ra)[AL]) {
        const bool first = g_ci < p.C1;
        const int cend = first ? p.C1 : Ctot;
        const bool kin = A_SPLIT ? g_ci < cend : g_ci + a_k < cend;      // split32: whole lines only (C % 32 == 0)
#pragma unroll
        for (int j = 0; j < ARS; ++j) {
            const float4* src = reinterpret_cast<const float4*>(
                static_cast<const float*>(first ? a_p1[j] : a_p2[j]) + g_ci);
            const float4 v = *((a_ok[j] && kin) ? src : g_zero4);   // (a local first: a direct struct copy into
            ra[j] = v;                                               //  the array defeats SROA -> scratch)
        }
        g_ci += BK;
        if (g_ci >= Ctot && g_tap + 1 < taps) {
            g_ci = 0;
            ++g_tap;
            set_tap(g_tap);
        }
    };

    // ---- B rows ([N][K], k contiguous)
    const float* b_ptr[BRS];
    bool b_ok[BRS];
#pragma unroll
    for (int j = 0; j < BRS; ++j) {
        const int row = b_r0 + b_rstep * j;
        const int n = n0 + row;
        b_ok[j] = n < Nb;
        b_ptr[j] = bp + (long long)(b_ok[j] ? n : 0) * p.ldb + b_k;
    }
    auto load_b = [&](float4 (&rb)[BL], int k0) {
        const bool kin = B_SPLIT ? k0 < p.K : k0 + b_k < p.K;
#pragma unroll
        for (int j = 0; j < BRS; ++j) {
            const float4* src = reinterpret_cast<const float4*>(b_ptr[j] + k0);
            const float4 v = *((b_ok[j] && kin) ? src : g_zero4);
            rb[j] = v;
        }
    };

    // fp32 float4 (4 k) -> hi / lo words at LDS element offset e
    auto put_f32 = [&](unsigned short* base, int e, float4 v) {
        uint2 hi, lo;
        if constexpr (TERMS == 1) {
            hi.x = pk_bf16(v.x, v.y);
            hi.y = pk_bf16(v.z, v.w);
            *reinterpret_cast<uint2*>(base + e) = hi;
        } else {
            split2(v.x, v.y, hi.x, lo.x);
            split2(v.z, v.w, hi.y, lo.y);
            *reinterpret_cast<uint2*>(base + e) = hi;
            *reinterpret_cast<uint2*>(base + PLANE_ELEMS + e) = lo;
        }
    };
    // LDS element offset of this thread's piece of row `row` for a split32 line: plane seg>>2, chunk (seg&3) swizzled
    auto split_dst = [&](int row) { return (seg >> 2) * PLANE_ELEMS + row * LDK + (((seg & 3) ^ ((row >> 2) & 3)) << 3); };
    auto f32_dst = [&](int row) { return row * LDK + (((seg >> 1) ^ ((row >> 2) & 3)) << 3) + (seg & 1) * 4; };
    auto store_tiles = [&](const float4 (&ra)[AL], const float4 (&rb)[BL], int buf) {
        unsigned short* base = smem + buf * PLANES * PLANE_ELEMS;
#pragma unroll
        for (int j = 0; j < ARS; ++j) {
            const int row = a_r0 + a_rstep * j;
            if constexpr (A_SPLIT) {
                if (PLANES == 2 || seg < 4) st16(base + split_dst(row), ra[j]);
            } else {
                float4 v = ra[j];
                v.x = fmaxf(v.x, v.x * slope);
                v.y = fmaxf(v.y, v.y * slope);
                v.z = fmaxf(v.z, v.z * slope);
                v.w = fmaxf(v.w, v.w * slope);
                put_f32(base, f32_dst(row), v);
            }
        }
#pragma unroll
        for (int j = 0; j < BRS; ++j) {
            const int row = BM + b_r0 + b_rstep * j;
            if constexpr (B_SPLIT) {
                if (PLANES == 2 || seg < 4) st16(base + split_dst(row), rb[j]);
            } else {
                put_f32(base, f32_dst(row), rb[j]);
            }
        }
    };

    f32x16 acc[MI][NI];
    zero_acc(acc);

    const int lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid - wm * WGN;
    const int lrow = lane & 31, lk = lane >> 5;
    const int a_row = (wm * WTM + lrow) * LDK, b_row = (BM + wn * WTN + lrow) * LDK;
    const int sw = (lrow >> 2) & 3;          // row swizzle of this lane's rows (tile offsets are multiples of 32)

    auto compute = [&](int buf) {
        const unsigned short* base = smem + buf * PLANES * PLANE_ELEMS;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            const int ch = ((ks * 2 + lk) ^ sw) << 3;
            bf16x8 ah[MI], bh[NI], al[MI], bl[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(base + a_row + i * 32 * LDK + ch);
                if constexpr (TERMS == 3) al[i] = *reinterpret_cast<const bf16x8*>(base + PLANE_ELEMS + a_row + i * 32 * LDK + ch);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                bh[j] = *reinterpret_cast<const bf16x8*>(base + b_row + j * 32 * LDK + ch);
                if constexpr (TERMS == 3) bl[j] = *reinterpret_cast<const bf16x8*>(base + PLANE_ELEMS + b_row + j * 32 * LDK + ch);
            }
            mma_kstep<TERMS>(acc, ah, al, bh, bl);
        }
    };

    // ---- main loop: PF register sets in flight, two LDS stages, one barrier per chunk
    static_assert(PF % 2 == 0 && PF >= 2, "prefetch depth");
    const int nchunks = (p.K + BK - 1) / BK;
    float4 ra[PF][AL], rb[PF][BL];
    set_tap(0);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        load_a(ra[u]);
        load_b(rb[u], u * BK);
    }
    store_tiles(ra[0], rb[0], 0);
    __syncthreads();
    for (int c = 0; c < nchunks; c += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            // chunk c + u sits in LDS stage u & 1; set u is free again
            load_a(ra[u]);
            load_b(rb[u], (c + u + PF) * BK);
            if (c + u < nchunks) compute(u & 1);
            store_tiles(ra[(u + 1) % PF], rb[(u + 1) % PF], (u + 1) & 1);
            __syncthreads();
        }
    }

    igemm_epilogue<MI, NI>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lrow, lk, coff, Nb, rpb);
}

template <int BM, int BN, int WGM, int WGN, int TERMS, bool AS, bool BS, int BKT, int PF>
void launch_one(const Ctx& ctx, const IGemm& p, int Nb) {
    const int ncols = p.N * (p.geglu ? 2 : 1);
    const int mtiles = (p.M + BM - 1) / BM, ntiles = (ncols + BN - 1) / BN;
    dim3 grid((unsigned)((long long)mtiles * ntiles), (unsigned)p.Z);
    constexpr int planes = TERMS == 1 ? 1 : 2;
    constexpr size_t lds = (size_t)2 * planes * (BM + BN) * BKT * sizeof(unsigned short);
    auto kern = igemm_bf16_kernel<BM, BN, WGM, WGN, TERMS, AS, BS, BKT, PF>;
    ensure_dynamic_lds(reinterpret_cast<const void*>(kern), ctx.device, (int)lds);
    hipLaunchKernelGGL(kern, grid, dim3(NT), lds, ctx.stream, p, ntiles, Nb);
}

template <int TERMS, bool AS, bool BS, int BKT>
void launch_tile(const Ctx& ctx, const IGemm& p, int cfg, int Nb) {
    // (PF = 4 was tried on the 64-wide tiles: no gain on L2-warm micro-benchmarks and 10 % slower inside the UNet,
    //  where its extra 32 VGPRs cost a wave per SIMD)
    switch (cfg) {
        case 0: launch_one<128, 128, 2, 2, TERMS, AS, BS, BKT, 2>(ctx, p, Nb); break;
        case 1: launch_one<128, 64, 2, 2, TERMS, AS, BS, BKT, 2>(ctx, p, Nb); break;
        case 2: launch_one<64, 64, 2, 2, TERMS, AS, BS, BKT, 2>(ctx, p, Nb); break;
        case 4: launch_one<128, 32, 4, 1, TERMS, AS, BS, BKT, 2>(ctx, p, Nb); break;
        default: launch_one<256, 32, 4, 1, TERMS, AS, BS, BKT, 2>(ctx, p, Nb); break;
    }
}

template <int TERMS, int BKT>
void launch_split(const Ctx& ctx, const IGemm& p, int cfg, int Nb) {
    if (p.a_split && p.b_split)
        launch_tile<TERMS, true, true, BKT>(ctx, p, cfg, Nb);
    else if (p.b_split)
        launch_tile<TERMS, false, true, BKT>(ctx, p, cfg, Nb);
    else
        launch_tile<TERMS, false, false, BKT>(ctx, p, cfg, Nb);
}

}  // namespace

// fp32 or half-split operands (split on the fly), and every bf16 problem under MAA_NO_DMA
void launch_igemm_bf16_reg(const Ctx& ctx, const IGemm& p, const IGemmPlan& pl) {
    if (ctx.dtype == 2)
        launch_split<1, 32>(ctx, p, pl.cfg, pl.Nb);
    else
        launch_split<3, 32>(ctx, p, pl.cfg, pl.Nb);
}

}  // namespace maa
