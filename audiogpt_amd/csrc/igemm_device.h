// Device-side vocabulary shared by the contraction engines and the kernels around them (device code only): vector types,
// counted waits, the address-space pointer types of the LDS-DMA copies, a compile-time loop and the XCD work orders.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace maa {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BK = 32;      // K depth of one LDS stage of the bf16 engines = one split32 line (32 bf16 hi | 32 bf16 lo)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

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

}  // namespace maa
