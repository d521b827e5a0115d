// Shared epilogue of the implicit-GEMM kernels.  The C/D fragment map of the 32x32 MFMA shapes is the same
// for every input dtype on gfx950 (lane l, register r: column l&31, row (r&3) + 8*(r>>2) + 4*(l>>5)), so the
// fp32 and the bf16-split kernels share this code.
#pragma once
#include "igemm_device.h"
#include "maa_internal.h"

namespace maa {

// erf for the GELU of the GEGLU epilogue: branch-free, ~25 VALU instructions (libm's erff costs ~100 and was a
// third of the ff.net.0 launch).  |x| < 1: x * P5(x^2); else 1 - exp(-Q7(|x|)) with |x| clamped to 4 (erf = 1 in
// fp32 beyond).  Polynomials are Chebyshev-node fits; max |error| against the fp64 erf is 1.2e-7 (0.5-1 ulp of
// the result near 1), measured over [-6, 6] in fp32 arithmetic.
__device__ __forceinline__ float fast_erff(float x) {
    const float t = fminf(fabsf(x), 4.0f);
    const float s = t * t;
    float r = -5.654105860e-04f;
    r = fmaf(r, s, 4.923277665e-03f);
    r = fmaf(r, s, -2.671638510e-02f);
    r = fmaf(r, s, 1.128036441e-01f);
    r = fmaf(r, s, -3.761234978e-01f);
    r = fmaf(r, s, 1.128379127e+00f);
    const float small = r * t;
    float q = 1.330939039e-05f;
    q = fmaf(q, t, -3.175720346e-04f);
    q = fmaf(q, t, 3.436867598e-03f);
    q = fmaf(q, t, -2.262198592e-02f);
    q = fmaf(q, t, 1.033189800e-01f);
    q = fmaf(q, t, 6.390933195e-01f);
    q = fmaf(q, t, 1.125925949e+00f);
    q = fmaf(q, t, 7.569686250e-04f);
    const float large = 1.0f - __builtin_amdgcn_exp2f(q * -1.4426950408889634f);
    return copysignf(t < 1.0f ? small : large, x);
}

// Pins a loaded value: the load is waited for HERE, once, in straight-line code.  Without it the compiler sinks the first
// use into the per-row `if (m < M)` branches and has to wait there -- with vmcnt(0), i.e. also for every store issued by
// the earlier rows, which turns a block's 16 stores into 16 dependent round trips.
__device__ __forceinline__ void settle(float& x) { asm volatile("" : "+v"(x)); }

// An output element in the split32 form (row pitch unchanged: every 32 columns = [32 bf16 hi | 32 bf16 lo]), from the
// accumulator layout of the MFMA epilogues, where lane l holds column n = ... + (l & 31): the two lanes of an
// even / odd column pair swap one half each (DPP quad_perm [1,0,3,2]) so that the even lane stores both hi halves and the odd
// lane both lo halves -- ONE 4-byte store per lane and element instead of two 2-byte stores.  Both lanes of a pair must be
// active (n even <-> lane even; callers guarantee N % 2 == 0 and a row condition that is uniform over the pair).
// (split_pair_word: the 4-byte word the lane stores -- both hi halves of the pair on the even lane, both lo halves on the odd one)
__device__ __forceinline__ unsigned split_pair_word(bool even, float v) {
    const __bf16 h = (__bf16)v;
    const unsigned hb = __builtin_bit_cast(unsigned short, h);
    const __bf16 l = (__bf16)(v - __builtin_bit_cast(float, hb << 16));
    const unsigned lb = __builtin_bit_cast(unsigned short, l);
    const unsigned mine = even ? lb : hb;                                  // what the partner stores
    const unsigned theirs = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mine, 0xB1, 0xF, 0xF, false);
    return even ? (hb | (theirs << 16)) : (theirs | (lb << 16));
}
__device__ __forceinline__ void store_split_pair(float* row, int n, float v) {
    const bool even = (n & 1) == 0;
    unsigned* o = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned short*>(row) + (n >> 5) * 64 + ((n & 31) & ~1) + (even ? 0 : 32));
    *o = split_pair_word(even, v);
}

// acc[MI][NI]: MI x NI fragments of 32x32 owned by this wave; (m_base, n_base) = first row / column of the wave.
// PAIR: plain fp32 output whose columns pair up (even width, even pitch, 8-byte aligned base): see the store loop
// RSEL: a sample has >= 32 rows (or there is no row add), so the row add of a block's row is one of two samples'
template <int MI, int NI, bool PAIR, bool RSEL>
__device__ __forceinline__ void igemm_epilogue_impl(const IGemm& p, f32x16 (&acc)[MI][NI], int m_base, int n_base,
                                                    int lrow, int lk, long long coff, int Nb, int rpb) {
    float* cp = p.c + coff;
    const float* resp = p.res ? p.res + coff : nullptr;
    if (p.geglu) {
        // packed columns: [32 value | 32 gate] per group of 64; output column = group*32 + j  (attention.py:42-44)
        if constexpr (NI % 2 == 0) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; j += 2) {
                    const int cpk = n_base + j * 32 + lrow;          // packed value column
                    const int ncol = (cpk >> 6) * 32 + lrow;         // output column
                    if (cpk + 32 < Nb && ncol < p.N) {
                        float bv = p.bias ? p.bias[cpk] : 0.f;
                        float bg = p.bias ? p.bias[cpk + 32] : 0.f;
                        settle(bv);
                        settle(bg);
                        // values first (straight-line: the bias loads are waited for once), stores after -- a load result
                        // first used inside a per-row branch makes every branch wait for all earlier stores as well
                        float outv[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float val = acc[i][j][r] * p.alpha + bv;
                            const float g = acc[i][j + 1][r] * p.alpha + bg;
                            const float gl = 0.5f * g * (1.f + fast_erff(g * 0.70710678118654752440f));
                            outv[r] = val * gl;
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = m_base + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                            if (m < p.M) {
                                if (p.c_split)
                                    store_split_pair(cp + (long long)m * p.ldc, ncol, outv[r]);
                                else
                                    cp[(long long)m * p.ldc + ncol] = outv[r];
                            }
                        }
                    }
                }
        }
        return;
    }
    // Every global read of a 32x32 block (time-embedding row add, residual, accumulate target) is issued before the block's
    // first store, so a block costs ONE memory round trip.  (Written as load-compute-store per element, the possible
    // aliasing of `res` / `c` makes the compiler wait for each load and each store in turn: 32-48 dependent round trips
    // per block -- 10-20 us per workgroup, which was the dominant cost of the short-K layers up to round 2.)
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        // sample index of the block's rows for the per-sample row add: 32 consecutive rows span at most two samples when a
        // sample has >= 32 rows (one division per block instead of one per row)
        const int mb = m_base + i * 32;
        const int b0 = (mb < p.M ? mb : p.M - 1) / rpb;      // (a block wholly past M reads the last sample's row, never one past it)
        const int nextb = (b0 + 1) * rpb;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int n = n_base + j * 32 + lrow;
            if (n < p.N) {
                float bias = p.bias ? p.bias[n] : 0.f;
                float ra[16], rs[16], cv[16];
                // unconditional loads from clamped rows under wave-uniform "is this term present" branches: straight-line
                // code, all of a block's reads in flight together
                long long mc[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mb + (r & 3) + 8 * (r >> 2) + 4 * lk;
                    mc[r] = m < p.M ? m : p.M - 1;
                    ra[r] = rs[r] = cv[r] = 0.f;
                }
                // (RSEL is a property of the instantiation: chosen per row at run time, even though rpb is wave-uniform, it compiled
                // to a branch around every load -- 500 basic blocks -- and as two alternative loops to a wait for every load in
                // flight where they join)
                if (p.rowadd) {
                    if constexpr (RSEL) {
                        const float* ra0 = p.rowadd + (long long)b0 * p.ld_rowadd + n;
#pragma unroll
                        for (int r = 0; r < 16; ++r) ra[r] = ra0[mc[r] < nextb ? 0 : p.ld_rowadd];
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) ra[r] = p.rowadd[(long long)((int)mc[r] / rpb) * p.ld_rowadd + n];
                    }
                }
                if (resp) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) rs[r] = resp[mc[r] * p.ldr + n];
                }
                if (p.accumulate && !p.c_split) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) cv[r] = cp[mc[r] * p.ldc + n];
                }
                // values first (straight-line: every read above is waited for once), then the stores
                settle(bias);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    settle(ra[r]);
                    settle(rs[r]);
                    settle(cv[r]);
                }
                // (blocks without an activation, the UNet's, skip the per-element chain of scalar branches that chooses it)
                float outv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j][r] * p.alpha + bias;
                    if (p.rowadd) v += ra[r];
                    if (resp) v += rs[r];
                    outv[r] = v;
                }
                if (p.act != 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = outv[r];
                        if (p.act == 1) v = tanhf(v);
                        else if (p.act == 2) v = fmaxf(v, 0.f);
                        else if (p.act == 3) v = 0.5f * v * (1.f + fast_erff(v * 0.70710678118654752440f));
                        else if (p.act == 4) v = v > 0.f ? v : v * p.act_slope;
                        outv[r] = v;
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = outv[r] * p.out_scale;
                    if (p.accumulate && !p.c_split) v += cv[r];
                    outv[r] = v;
                }
                if constexpr (PAIR) {
                    // fp32 rows, two columns per lane: the lanes of an even / odd column pair swap one value per pair of
                    // rows (DPP), the even lane stores columns (n, n + 1) of the even row, the odd lane those of the odd row
                    // -- 8 eight-byte stores per lane and block instead of 16 four-byte ones (the tail of these kernels is
                    // store-issue-bound)
                    const bool even = (lrow & 1) == 0;
#pragma unroll
                    for (int rp = 0; rp < 8; ++rp) {
                        const float keep = even ? outv[2 * rp] : outv[2 * rp + 1];
                        const float give = even ? outv[2 * rp + 1] : outv[2 * rp];
                        const float got = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, give), 0xB1, 0xF, 0xF, false));
                        const int r = 2 * rp + (even ? 0 : 1);
                        const int m = mb + (r & 3) + 8 * (r >> 2) + 4 * lk;
                        if (m < p.M) {
                            const f32x2 v2 = even ? f32x2{keep, got} : f32x2{got, keep};
                            *reinterpret_cast<f32x2*>(cp + (long long)m * p.ldc + (n & ~1)) = v2;
                        }
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = mb + (r & 3) + 8 * (r >> 2) + 4 * lk;
                        if (m < p.M) {
                            if (p.c_split)
                                store_split_pair(cp + (long long)m * p.ldc, n, outv[r]);
                            else
                                cp[(long long)m * p.ldc + n] = outv[r];
                            if (p.c2) {
                                const float w = outv[r] > 0.f ? outv[r] : outv[r] * p.c2_slope;
                                store_split_pair(p.c2 + coff + (long long)m * p.ldc2, n, w);
                            }
                        }
                    }
                }
            }
        }
    }
}

template <int MI, int NI>
__device__ __forceinline__ void igemm_epilogue(const IGemm& p, f32x16 (&acc)[MI][NI], int m_base, int n_base, int lrow,
                                               int lk, long long coff, int Nb, int rpb) {
    const bool pair = !p.geglu && !p.c_split && p.c2 == nullptr && (p.N & 1) == 0 && (p.ldc & 1) == 0 && (coff & 1) == 0 &&
                      (reinterpret_cast<uintptr_t>(p.c) & 7) == 0;
    const bool rsel = !(p.rowadd && rpb < 32);       // (false: images of a few pixels, one division per row)
    if (pair && rsel)
        igemm_epilogue_impl<MI, NI, true, true>(p, acc, m_base, n_base, lrow, lk, coff, Nb, rpb);
    else if (pair)
        igemm_epilogue_impl<MI, NI, true, false>(p, acc, m_base, n_base, lrow, lk, coff, Nb, rpb);
    else if (rsel)
        igemm_epilogue_impl<MI, NI, false, true>(p, acc, m_base, n_base, lrow, lk, coff, Nb, rpb);
    else
        igemm_epilogue_impl<MI, NI, false, false>(p, acc, m_base, n_base, lrow, lk, coff, Nb, rpb);
}

// ------------------------------------------------------------------------------------------ epilogue kinds fixed at compile time
// The function above carries every feature as a run-time flag and decides it per 32x32 block; what a transformer linear needs of it
// is a few hundred instructions.  A launcher that knows its IGemm picks one of these kinds (igemm_epi_kind) and the kernel is
// instantiated with it; GENERIC is the function above and takes everything the other kinds do not.  The arithmetic of the fast
// kinds is the generic expression with the absent terms left out -- alpha == 1 and out_scale == 1 are conditions of every fast
// kind, x * 1.0f is exact and the build has -ffp-contract=off -- so a launch returns the same bits under either.
//   PLAIN   acc + bias (+ residual), fp32 pair stores           q / k / v, to_out, proj_in / proj_out, ff.net.2
//   SPLIT   the same, written as split32 lines (c_split)
//   GEGLU   value * gelu(gate), fp32 or split32 output          ff.net.0
enum class Epi : int { GENERIC = 0, PLAIN = 1, SPLIT = 2, GEGLU = 3 };

// Kind of a launch whose output starts at p.c (Z == 1).  The fast kinds address a 32x32 block as one 64-bit base plus 32-bit
// offsets of up to 32 rows, hence the pitch limits.
inline Epi igemm_epi_kind(const IGemm& p) {
    const bool pitches = p.ldc > 0 && p.ldc < (1 << 24) && p.ldr >= 0 && p.ldr < (1 << 24);
    if (!pitches || p.Z != 1 || p.M <= 0 || p.alpha != 1.f || p.out_scale != 1.f || p.rowadd || p.act != 0 || p.accumulate || p.c2)
        return Epi::GENERIC;
    if (p.geglu) return p.res ? Epi::GENERIC : Epi::GEGLU;
    if (p.c_split) return (p.N & 1) == 0 ? Epi::SPLIT : Epi::GENERIC;
    const bool pair = (p.N & 1) == 0 && (p.ldc & 1) == 0 && (reinterpret_cast<uintptr_t>(p.c) & 7) == 0;
    return pair ? Epi::PLAIN : Epi::GENERIC;
}

__device__ __forceinline__ constexpr unsigned frag_row(int r) { return (unsigned)((r & 3) + 8 * (r >> 2)); }

// One wave's blocks.  FULL: the wave's MI x NI blocks lie wholly inside M and N (no row clamps, no guards); otherwise the guarded
// form, whose reads come from clamped rows as in the generic function.  (mb0, nb0) are wave-uniform; a block is addressed as a
// uniform base + this lane's 32-bit offset, and the offset of a fragment row is a uniform multiple of the pitch on top of the
// lane's own (4 lk) * pitch + column, formed once.  All reads of a block are issued before its first store (settle).
template <int MI, int NI, Epi KIND, bool FULL, bool RES>
__device__ __forceinline__ void igemm_epilogue_fast_body(const IGemm& p, f32x16 (&acc)[MI][NI], int mb0, int nb0, int lrow, int lk,
                                                         int Nb) {
    const bool even = (lrow & 1) == 0;
    const unsigned ldc = (unsigned)p.ldc, ldr = (unsigned)p.ldr;
    const unsigned lane_f32 = 4u * lk * ldc + lrow;                                   // fp32 element (row 4 lk, column lrow)
    const unsigned lane_pair = (4u * lk + (even ? 0u : 1u)) * ldc + (lrow & ~1);      // pair store: even lane the even row, odd lane the odd row
    const unsigned lane_split = 4u * lk * ldc + (lrow >> 1) + (even ? 0u : 16u);      // split32 word: hi pairs | lo pairs of the 32 columns
    const unsigned lane_res = 4u * lk * ldr + lrow;
    if constexpr (KIND == Epi::GEGLU) {
        // packed columns: [32 value | 32 gate] per group of 64; output column = group*32 + j
        static_assert(NI % 2 == 0, "GEGLU pairs a value block with a gate block");
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int mb = mb0 + i * 32;
            if (!FULL && mb >= p.M) break;
#pragma unroll
            for (int j = 0; j < NI; j += 2) {
                const int cb = nb0 + j * 32, ob = (cb >> 6) * 32;
                const int cpk = cb + lrow;
                if (FULL || (cpk + 32 < Nb && ob + lrow < p.N)) {
                    float bv = p.bias ? p.bias[cpk] : 0.f;
                    float bg = p.bias ? p.bias[cpk + 32] : 0.f;
                    settle(bv);
                    settle(bg);
                    float outv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float val = acc[i][j][r] + bv;
                        const float g = acc[i][j + 1][r] + bg;
                        const float gl = 0.5f * g * (1.f + fast_erff(g * 0.70710678118654752440f));
                        outv[r] = val * gl;
                    }
                    float* blk = p.c + ((long long)mb * ldc + ob);
                    if (p.c_split) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned w = split_pair_word(even, outv[r]);
                            if (FULL || mb + (int)frag_row(r) + 4 * lk < p.M) reinterpret_cast<unsigned*>(blk)[lane_split + frag_row(r) * ldc] = w;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (FULL || mb + (int)frag_row(r) + 4 * lk < p.M) blk[lane_f32 + frag_row(r) * ldc] = outv[r];
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int mb = mb0 + i * 32;
            if (!FULL && mb >= p.M) break;
            const unsigned last = (unsigned)(p.M - 1 - mb);        // (guarded form) last row of the block that exists
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int nb = nb0 + j * 32;
                if (FULL || nb + lrow < p.N) {
                    float bias = p.bias ? p.bias[nb + lrow] : 0.f;
                    float rs[16];
                    if constexpr (RES) {
                        const float* rb = p.res + ((long long)mb * ldr + nb);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            if constexpr (FULL) {
                                rs[r] = rb[lane_res + frag_row(r) * ldr];
                            } else {
                                const unsigned row = frag_row(r) + 4u * lk;
                                rs[r] = rb[(row < last ? row : last) * ldr + lrow];
                            }
                        }
                    }
                    settle(bias);
                    float outv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[i][j][r] + bias;
                        if constexpr (RES) {
                            settle(rs[r]);
                            v += rs[r];
                        }
                        outv[r] = v;
                    }
                    float* blk = p.c + ((long long)mb * ldc + nb);
                    if constexpr (KIND == Epi::PLAIN) {
                        // two columns per lane, as in the generic function's PAIR form
#pragma unroll
                        for (int rp = 0; rp < 8; ++rp) {
                            const float keep = even ? outv[2 * rp] : outv[2 * rp + 1];
                            const float give = even ? outv[2 * rp + 1] : outv[2 * rp];
                            const float got = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, give), 0xB1, 0xF, 0xF, false));
                            const f32x2 v2 = even ? f32x2{keep, got} : f32x2{got, keep};
                            if (FULL || mb + (int)frag_row(2 * rp) + 4 * lk + (even ? 0 : 1) < p.M)
                                *reinterpret_cast<f32x2*>(blk + (lane_pair + frag_row(2 * rp) * ldc)) = v2;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned w = split_pair_word(even, outv[r]);
                            if (FULL || mb + (int)frag_row(r) + 4 * lk < p.M) reinterpret_cast<unsigned*>(blk)[lane_split + frag_row(r) * ldc] = w;
                        }
                    }
                }
            }
        }
    }
}

// (m_base, n_base) = first row / column of the wave, as for igemm_epilogue.  One wave-uniform decision per tile: a wave wholly
// past M or N has nothing to write; one wholly inside takes the unguarded body.
template <int MI, int NI, Epi KIND>
__device__ __forceinline__ void igemm_epilogue_fast(const IGemm& p, f32x16 (&acc)[MI][NI], int m_base, int n_base, int lrow, int lk,
                                                    int Nb) {
    static_assert(KIND != Epi::GENERIC, "the generic kind is igemm_epilogue");
    const int mb0 = __builtin_amdgcn_readfirstlane(m_base), nb0 = __builtin_amdgcn_readfirstlane(n_base);
    if (mb0 >= p.M) return;
    bool full = mb0 + MI * 32 <= p.M;
    if constexpr (KIND == Epi::GEGLU) {
        // every lane's guard (cpk + 32 < Nb, output column < N) holds iff the last lane's of the last block pair does
        const int cpk = nb0 + (NI - 2) * 32 + 31;
        if (nb0 + 32 >= Nb) return;
        full = full && cpk + 32 < Nb && (cpk >> 6) * 32 + 31 < p.N;
        if (full)
            igemm_epilogue_fast_body<MI, NI, KIND, true, false>(p, acc, mb0, nb0, lrow, lk, Nb);
        else
            igemm_epilogue_fast_body<MI, NI, KIND, false, false>(p, acc, mb0, nb0, lrow, lk, Nb);
    } else {
        if (nb0 >= p.N) return;
        full = full && nb0 + NI * 32 <= p.N;
        if (p.res) {
            if (full)
                igemm_epilogue_fast_body<MI, NI, KIND, true, true>(p, acc, mb0, nb0, lrow, lk, Nb);
            else
                igemm_epilogue_fast_body<MI, NI, KIND, false, true>(p, acc, mb0, nb0, lrow, lk, Nb);
        } else {
            if (full)
                igemm_epilogue_fast_body<MI, NI, KIND, true, false>(p, acc, mb0, nb0, lrow, lk, Nb);
            else
                igemm_epilogue_fast_body<MI, NI, KIND, false, false>(p, acc, mb0, nb0, lrow, lk, Nb);
        }
    }
}

}  // namespace maa
