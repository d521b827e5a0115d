// Which engine runs a contraction, with which tile and how many K slices -- and the one path that launches it.
//
//   launch_igemm = fill in the zero page -> igemm_plan (pure host code, launches nothing) -> borrow the split-K slabs from the
//   arena -> profile row -> the engine's launch_* -> give the slabs back.
//
// The cascade of igemm_plan, in this order:
//   exact-fp32 context, or a problem the bf16 engines cannot take (B not k-contiguous, unaligned rows)   -> F32       igemm_f32.hip
//   both operands split32 and a 128x128 / 128x64 / 64x64 tile (unless MAA_NO_DMA):
//       stride-1 "same" convolutions whose rings fit the LDS                                            -> PP        igemm_pp.hip
//       1x1 / Linear whose 256-row tiles fill the chip                                                   -> PP1       igemm_pp.hip
//       long K (>= 2048)                                                                                 -> DMA2      igemm_dma2.hip
//       everything else                                                                                  -> DMA       igemm_dma.hip
//   fp32 or half-split operands, N <= 32                                                                 -> BF16_REG  igemm_bf16.hip
// Eligibility that needs an engine's geometry (ring sizes, tile counts) stays beside that geometry, behind igemm_*_takes.
// The tile width and the number of K slices are functions of the layer only (K and the packed N, never M): a sample's result does
// not depend on the batch it was computed in.
#include "maa_internal.h"

namespace maa {

namespace {

bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// Aligned gather of an fp32 A operand: `chunk`-channel pieces never straddle a tap or a source and the float4 loads are aligned
// (single source, K % 4 != 0: the last float4 over-reads up to 3 floats of the same row, which must exist and be finite -- e.g.
// the zeroed padding columns of the attention scores; they meet zero rows of B)
bool gather_aligned(const IGemm& p, int chunk) {
    const int taps = p.KH * p.KW, Ctot = p.C1 + p.C2;
    bool fast = (taps == 1 ? (p.C2 == 0 ? (Ctot % 4 == 0 || p.lda1 >= (Ctot + 3) / 4 * 4)
                                        : (p.C1 % chunk == 0 && Ctot % 4 == 0))
                           : (Ctot % chunk == 0 && p.C1 % chunk == 0)) &&
                p.lda1 % 4 == 0 && al16(p.a1) && p.a_so % 4 == 0 && p.a_si % 4 == 0;
    if (p.C2 > 0) fast = fast && p.lda2 % 4 == 0 && al16(p.a2);
    return fast;
}

// tile of the F32 / BF16_REG / DMA engines by index
constexpr int kTileM[5] = {128, 128, 64, 256, 128}, kTileN[5] = {128, 64, 64, 32, 32};

struct TileKnobs {
    double eff[3] = {1.00, 0.92, 0.80};       // per-block efficiency of 128x128 / 128x64 / 64x64
    double conc[3] = {0.55, 0.85, 1.00};      // latency hiding with 1 / 2 / >=3 co-resident blocks per CU
};

// The bf16 modes' part of the cascade; false: the problem goes to the exact-fp32 kernel.
bool plan_bf16(const Ctx& ctx, const IGemm& p, IGemmPlan& pl) {
    if (!p.b_nk) {
        MAA_CHECK(!p.a_split && !p.b_split, "split operands need the k-contiguous bf16 engine");
        return false;
    }
    const int taps = p.KH * p.KW, Ctot = p.C1 + p.C2;
    bool fast;
    if (p.a_split)      // split32 lines: whole 32-channel groups, rows pitched like their fp32 form
        fast = p.C2 == 0 && Ctot % 32 == 0 && p.lda1 % 32 == 0 && al16(p.a1) && p.Z == 1 && p.a_act == 0;
    else
        fast = gather_aligned(p, 32);
    if (p.b_split)
        fast = fast && p.ldb % 32 == 0 && al16(p.b) && p.K % 32 == 0 && p.ldb >= p.K && p.Z == 1;
    else
        fast = fast && p.ldb % 4 == 0 && al16(p.b) && p.b_so % 4 == 0 && p.b_si % 4 == 0 && p.ldb >= (p.K + 3) / 4 * 4;
    fast = fast && p.K == taps * Ctot && (p.a_act == 0 || p.a_act == 1);
    if (!fast) {
        MAA_CHECK(!p.a_split && !p.b_split, "split operand given to a problem the bf16 engine cannot take");
        return false;
    }
    MAA_CHECK(!(p.c_split || p.c2) || p.N % 32 == 0, "split32 outputs are whole 32-channel lines");
    const int ncols = p.N * (p.geglu ? 2 : 1);
    pl.fast = true;
    pl.Nb = ncols;       // rows of B that exist
    if (p.geglu) {
        if (ncols % 64 != 0) return false;
        pl.cfg = 0;
    } else if (ncols <= 32) {
        // 256-row tiles; 128-row ones while those would leave most of the chip idle (the UNet's 320 -> 4 output convolution:
        // 49 workgroups of 90 chunks each).  No K split either way: the two tiles give bit-identical results.
        pl.cfg = (long long)((p.M + 255) / 256) * p.Z < 128 ? 4 : 3;
    } else {
        pl.cfg = choose_tile(p.M, ncols, p.Z, true, ctx.kept_full() ? 1 : 0);
    }
    pl.engine = IGemmPlan::BF16_REG;
    // both bf16 modes: split32 x split32 problems go to the LDS-DMA engines (plain bf16: the hi halves are the operands);
    // MAA_NO_DMA (tests): the same arithmetic with register staging
    if (p.a_split && p.b_split && pl.cfg < 3 && !ctx.tune.no_dma) {
        if (!igemm_pp_takes(ctx, p, pl) && !igemm_pp1_takes(ctx, p, pl) && !igemm_dma2_takes(ctx, p, pl)) igemm_dma_takes(ctx, p, pl);
    }
    if (pl.S > 1) {      // slabs of the split-K engines: S fp32 copies of every tile (slab_floats, igemm_device.h: one float per tile
                         // element), borrowed from the arena for the two launches; the engine's launcher checks this size against its tile
        const int bm = pl.engine == IGemmPlan::DMA2 ? 128 : 256, bn = pl.engine == IGemmPlan::DMA2 ? 128 : pl.bn;
        const long long tiles = (long long)((p.M + bm - 1) / bm) * ((ncols + bn - 1) / bn);
        pl.slab_floats = (size_t)(tiles * pl.S * bm * bn);
    }
    return true;
}

// Profile row of a planned launch: the kernel family and tile, or with `detail` the engine, tile, slices and problem shape
// (bench.py's roofline and the dispatch tests key on these).  Work = 2 M N K per batch entry (GEGLU computes 2N columns);
// traffic = weights once + output once.
const char* plan_row(const Ctx& ctx, const IGemm& p, const IGemmPlan& pl, char (&buf)[64], double& flops, double& bytes) {
    const int ncols = p.N * (p.geglu ? 2 : 1), taps = p.KH * p.KW;
    flops = 2.0 * p.M * (double)ncols * p.K * p.Z;
    bytes = 4.0 * ((double)p.K * ncols + (double)p.M * p.N * p.Z);
    const bool detail = ctx.prof && ctx.prof->detail;
    const char* mode = ctx.dtype == 2 ? "_bf16" : "_bf16x3";
    const char* splitk = pl.S > 1 ? ",splitK" : "";
    switch (pl.engine) {
        case IGemmPlan::PP:
        case IGemmPlan::PP1: {
            const bool one = pl.engine == IGemmPlan::PP1;
            if (detail) std::snprintf(buf, sizeof(buf), "p%c%d M%d N%d K%d S%d", one ? 'q' : 'p', pl.bn, p.M, ncols, p.K, pl.S);
            else std::snprintf(buf, sizeof(buf), "igemm_pp%s%s<256x%d%s>", one ? "1" : "", mode, pl.bn, splitk);
            break;
        }
        case IGemmPlan::DMA2:
            if (detail) std::snprintf(buf, sizeof(buf), "b2 M%d N%d K%d t%d", p.M, ncols, p.K, taps);
            else std::snprintf(buf, sizeof(buf), "igemm_dma2%s<128x128%s>", mode, splitk);
            break;
        case IGemmPlan::DMA:
        case IGemmPlan::BF16_REG: {
            const bool dma = pl.engine == IGemmPlan::DMA;
            if (detail) std::snprintf(buf, sizeof(buf), "b%c%d M%d N%d K%d t%d Z%d", dma ? 'd' : 'g', pl.cfg, p.M, ncols, p.K, taps, p.Z);
            else std::snprintf(buf, sizeof(buf), "igemm%s%s<%dx%d>", dma ? "_dma" : "", mode, kTileM[pl.cfg], kTileN[pl.cfg]);
            break;
        }
        default:
            if (detail) std::snprintf(buf, sizeof(buf), "ig%d M%d N%d K%d t%d Z%d%s", pl.cfg, p.M, ncols, p.K, taps, p.Z, p.b_nk ? "T" : "");
            else std::snprintf(buf, sizeof(buf), "igemm_f32<%dx%d>", kTileM[pl.cfg], kTileN[pl.cfg]);
            break;
    }
    return buf;
}

}  // namespace

// Tile choice shared by the fp32 and bf16 engines: 0 = 128x128, 1 = 128x64, 2 = 64x64 (the 32-wide tiles are chosen by igemm_plan
// for N <= 32).  Cost = CU-rounds x tile area / (tile efficiency x latency hiding at that many co-resident blocks per CU).
int choose_tile(long long M, long long N, int Z, bool bf16, int mode) {
    static const TileKnobs k;
    const int max_occ[3] = {bf16 ? 2 : 3, bf16 ? 2 : 4, 4};   // blocks per CU allowed by LDS / registers
    int best = 0;
    double best_cost = 1e300;
    for (int c = 0; c < 3; ++c) {
        const int bm = kTileM[c], bn = kTileN[c];
        const long long blocks = ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * Z;
        const long long per_cu = (blocks + 255) / 256;
        const int co = (int)(per_cu < max_occ[c] ? per_cu : max_occ[c]);
        // mode 1: the chip is kept full from outside (other contexts' launches run on the CUs this one leaves idle), so what a
        // launch costs is the sum of its workgroups' time, padding included -- not the rounds its own grid makes
        const double cost = mode == 1 ? (double)blocks * bm * bn / k.eff[c]
                                      : (double)per_cu * bm * bn / (k.eff[c] * k.conc[co >= 3 ? 2 : co - 1]);
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

// slices for a K of `nchunks` chunks such that no slice is empty: the largest S' <= S with ceil(nchunks / ceil(nchunks / S')) == S'
int fit_slices(int nchunks, int S) {
    if (S < 1) S = 1;
    if (S > nchunks) S = nchunks;
    for (; S > 1; --S) {
        const int cps = (nchunks + S - 1) / S;
        if ((nchunks + cps - 1) / cps == S) break;
    }
    return S;
}

IGemmPlan igemm_plan(const Ctx& ctx, const IGemm& p) {
    IGemmPlan pl;
    // (no model asks for both: the epilogue reads no accumulate target when it writes split32 lines, so the sum would be dropped)
    MAA_CHECK(!(p.accumulate && p.c_split), "split32 output cannot accumulate");
    // (likewise the GEGLU branch of the epilogue is value * gelu(gate) of alpha * acc + bias and nothing else)
    MAA_CHECK(!p.geglu || (!p.rowadd && !p.res && p.act == 0 && p.out_scale == 1.f && !p.accumulate && !p.c2),
              "GEGLU takes no row add, residual, activation, output scale, accumulate or second output");
    // precision mode of the context: 1 = bf16x3 split, 2 = plain bf16 operands; problems the bf16 engines cannot take run on the
    // exact-fp32 kernel.  (The bf16 part also runs in the workspace dry run: its split-K slabs come from the arena.)
    if (ctx.dtype != 0 && plan_bf16(ctx, p, pl)) return pl;
    pl = IGemmPlan();
    if (ctx.ws.dry) return pl;
    MAA_CHECK(p.M > 0 && p.N > 0 && p.K > 0, "empty igemm");
    MAA_CHECK(!p.c_split, "split32 output asked of a problem only the fp32 engine can take");
    MAA_CHECK(!p.c2, "second (split32) output asked of a problem only the fp32 engine can take");      // (its epilogue writes none)
    const int taps = p.KH * p.KW, Ctot = p.C1 + p.C2;
    MAA_CHECK(p.K <= taps * Ctot && p.K > (taps - 1) * Ctot, "igemm K mismatch");
    MAA_CHECK(p.a_act == 0 || p.a_act == 1, "igemm A activation");
    pl.fast = gather_aligned(p, 16);      // else the per-element gather (first convolutions with Cin = 1, 4, 9, 80)
    if (p.Z > 1) MAA_CHECK(p.C2 == 0, "batched igemm takes one A source");
    MAA_CHECK(pl.fast || p.K == taps * Ctot, "padded K needs the aligned gather");
    // columns that may be read from B: packed weights are zero-padded to a multiple of 32
    const int ncols = p.N * (p.geglu ? 2 : 1);
    pl.Nb = ncols;
    MAA_CHECK(p.ldb % 4 == 0 && al16(p.b) && p.b_so % 4 == 0 && p.b_si % 4 == 0, "B operand alignment");
    if (!p.b_nk) {
        pl.Nb = (ncols + 3) / 4 * 4;
        if (pl.Nb > p.ldb) pl.Nb = p.ldb / 4 * 4;
    } else {
        MAA_CHECK(p.ldb >= (p.K + 3) / 4 * 4, "B [N][K] rows must be padded to a multiple of 4");
    }
    if (p.geglu) {
        MAA_CHECK(ncols % 64 == 0, "geglu needs packed N multiple of 64");
        pl.cfg = 0;
    } else if (ncols <= 32) {
        pl.cfg = 3;
    } else {
        pl.cfg = choose_tile(p.M, ncols, p.Z, false);
    }
    return pl;
}

void launch_igemm(const Ctx& ctx, const IGemm& p_in) {
    IGemm p = p_in;
    p.zeros = ctx.zeros;
    MAA_CHECK(p.zeros != nullptr, "context has no zero page");
    const IGemmPlan pl = igemm_plan(ctx, p);
    // split-K slabs are borrowed from the arena for the duration of the launches (stream order protects them from later
    // borrowers); the arena's dry run counts them and launches nothing
    const size_t mk = ctx.ws.mark();
    float* part = pl.slab_floats ? ctx.ws.alloc_f(pl.slab_floats) : nullptr;
    if (!ctx.ws.dry) {
        char row[64];
        double flops, bytes;
        const char* name = plan_row(ctx, p, pl, row, flops, bytes);
        ProfScope prof(ctx, name, flops, bytes);
        switch (pl.engine) {
            case IGemmPlan::PP: launch_igemm_pp(ctx, p, pl, part); break;
            case IGemmPlan::PP1: launch_igemm_pp1(ctx, p, pl, part); break;
            case IGemmPlan::DMA2: launch_igemm_dma2(ctx, p, pl, part); break;
            case IGemmPlan::DMA: launch_igemm_dma(ctx, p, pl); break;
            case IGemmPlan::BF16_REG: launch_igemm_bf16_reg(ctx, p, pl); break;
            case IGemmPlan::F32: launch_igemm_f32(ctx, p, pl); break;
        }
        MAA_HIP(hipGetLastError());
    }
    ctx.ws.release(mk);
}

}  // namespace maa
