// Device-side vocabulary shared by the contraction engines and the kernels around them (device code only): vector types,
// counted waits, the address-space pointer types of the LDS-DMA copies, a compile-time loop, the XCD work orders, and what the bf16
// engines do alike: the k-step, the fragment slots of a split32 line in LDS, the split-K slab.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace maa {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// split32 of a pair of floats: hi = bf16(v) of both packed in one dword (low half = a), lo = bf16(v - hi) likewise
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    f32x2 f = {a, b};
    bf16x2 h = __builtin_convertvector(f, bf16x2);      // v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
    hi = pk_bf16(a, b);
    lo = pk_bf16(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}

constexpr int BK = 32;     // K depth of one LDS stage of the bf16 engines = one split32 line (32 bf16 hi | 32 bf16 lo)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// operands of __builtin_amdgcn_global_load_lds
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// compile-time loop: f(std::integral_constant<int, I>) for I in [0, N) -- indices into register arrays stay literal
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// XCD-contiguous work order.  Workgroup `bid` of a 1-D grid of `n` runs on XCD bid % 8 (observed placement, used for speed only:
// results never depend on it); XCD x takes the x-th contiguous eighth of the work items, workgroup by workgroup.  Every engine
// gives its tiles this order (M-major, N-tiles fastest), so the N-tiles of one M-tile and the neighbouring M-tiles -- which share
// A rows through the conv halo -- meet in one L2 (4 MB, not shared between XCDs) instead of being fetched over the fabric once
// per XCD; the normalisation / attention / reduce launches use it too, so that the rows a workgroup reads were written, and the
// rows it writes will be read, by workgroups of the SAME XCD.  Bijective for any grid size.
__device__ __forceinline__ int xcd_contiguous(int bid, int n) {
    const int xcd = bid & 7, q = n >> 3, r = n & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// The same order for persistent workgroups (a grid smaller than its `items`): this workgroup's XCD owns items [lo, lo + cnt) and
// the workgroup runs lo + first, lo + first + step, ... -- `step` = the XCD's workgroups, so at any time they work on neighbours.
struct XcdRange {
    int lo, cnt, step, first;
};
__device__ __forceinline__ XcdRange xcd_range(int items) {
    const int G = (int)gridDim.x, xcd = blockIdx.x & 7, q = items >> 3, r = items & 7;
    XcdRange w;
    w.lo = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    w.cnt = q + (xcd < r ? 1 : 0);
    w.step = (G - xcd + 7) >> 3;
    w.first = (int)(blockIdx.x >> 3);
    return w;
}

// ---- what the bf16 engines share: the k-step, the accumulators, the LDS-DMA engines' fragment slots, the split-K slab

// One 16-deep k-step of a wave's MI x NI accumulators.  NUMERICAL CONTRACT of the bf16 engines: per accumulator the products
// are issued lo.hi, hi.lo, hi.hi (TERMS = 1: hi.hi alone), k ascending -- every engine calls this (igemm_dma2.hip's second
// k-step spells the same order out to interleave its copies), which is what makes them bit-identical to each other.  Term-major:
// the three products of one accumulator are MI NI - 1 MFMAs of the other accumulators apart, so results do not depend on the
// tile shape and no accumulator chain waits for itself.
template <int TERMS, int MI, int NI>
__device__ __forceinline__ void mma_kstep(f32x16 (&acc)[MI][NI], const bf16x8 (&ah)[MI], const bf16x8 (&al)[MI],
                                          const bf16x8 (&bh)[NI], const bf16x8 (&bl)[NI]) {
    if constexpr (TERMS == 3) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
}

template <int MI, int NI>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MI][NI]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// A split32 line in LDS (the LDS-DMA engines): 16-byte slot s of row r is stored at slot s ^ ((r >> 1) & 7).  off[plane][k-step]
// = byte offset inside its row of this lane's operand piece (plane 0 = hi, 1 = lo); tile offsets are multiples of 32 rows, so
// the swizzle depends on lrow only.
__device__ __forceinline__ void frag_slot_offsets(int lrow, int lk, int (&off)[2][2]) {
    const int swz = (lrow >> 1) & 7;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) off[pl][ks] = ((pl * 4 + ks * 2 + lk) ^ swz) << 4;
}

// The fragments of k-step ks in the order igemm_dma.hip and igemm_dma2.hip read them: al, bh, ah, bl (the first products' operands first)
template <int TERMS, int MI, int NI>
__device__ __forceinline__ void read_frags_kstep(const char* base, int a_row, int b_row, const int (&off)[2][2], int ks,
                                                 bf16x8 (&ah)[MI], bf16x8 (&al)[MI], bf16x8 (&bh)[NI], bf16x8 (&bl)[NI]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
        if constexpr (TERMS == 3) al[i] = *reinterpret_cast<const bf16x8*>(base + a_row + i * 4096 + off[1][ks]);
#pragma unroll
    for (int j = 0; j < NI; ++j) bh[j] = *reinterpret_cast<const bf16x8*>(base + b_row + j * 4096 + off[0][ks]);
#pragma unroll
    for (int i = 0; i < MI; ++i) ah[i] = *reinterpret_cast<const bf16x8*>(base + a_row + i * 4096 + off[0][ks]);
#pragma unroll
    for (int j = 0; j < NI; ++j)
        if constexpr (TERMS == 3) bl[j] = *reinterpret_cast<const bf16x8*>(base + b_row + j * 4096 + off[1][ks]);
}

// Split-K slab of one (slice, tile), written by a workgroup of NTH threads with MI x NI accumulators per wave and read back by
// splitk_reduce_kernel's twin threads: [MI NI blocks][4 register quads][NTH threads][4 floats] -- every store instruction of a
// wave writes 1 KB contiguous.  One float per tile element: slab_floats = BM BN (what igemm_plan borrows per slice and tile).
// slab_thread: thread tid's quad 0 of block 0 in slab number `slab`; slab_quad: floats from there to its quad `quad` of block blk.
constexpr long long slab_floats(int MI, int NI, int NTH) { return (long long)(MI * NI * 4) * NTH * 4; }
template <int MI, int NI, int NTH, class T>
__device__ __forceinline__ T* slab_thread(T* part, long long slab, int tid) {
    return part + (slab * (MI * NI * 4) * NTH + tid) * 4;
}
template <int NTH>
__device__ __forceinline__ long long slab_quad(int blk, int quad) {
    return (long long)(blk * 4 + quad) * NTH * 4;
}
template <int MI, int NI, int NTH>
__device__ __forceinline__ void store_slab(float* part, int slab, int tid, const f32x16 (&acc)[MI][NI]) {
    float* pp = slab_thread<MI, NI, NTH>(part, slab, tid);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                *reinterpret_cast<f32x4*>(pp + slab_quad<NTH>(i * NI + j, q)) = v;
            }
}

}  // namespace maa
