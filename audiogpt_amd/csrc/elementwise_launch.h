// Launch of a grid-stride elementwise kernel: the grid and the one launch macro of misc.hip, diffsinger.hip, sampler_steps.hip,
// split.hip and spectral.hip.
#pragma once
#include "maa_internal.h"

namespace maa {

// blocks of 256 threads for n elements, at most max_blocks (the kernels' loops stride over the rest), at least one
inline dim3 grid_for(long long n, long long max_blocks = 8192) {
    long long b = (n + 255) / 256;
    if (b > max_blocks) b = max_blocks;
    if (b < 1) b = 1;
    return dim3((unsigned)b);
}

}  // namespace maa

// the body of a launcher `void launch_x(const Ctx& ctx, ...)`: nothing on a dry (sizing) pass, the kernel's own name as the
// profile's row
#define MAA_LAUNCH1(kern, n, ...)                                                            \
    if (ctx.ws.dry) return;                                                                  \
    ProfScope prof(ctx, #kern, 0.0, 8.0 * (double)(n));                                      \
    hipLaunchKernelGGL(kern, grid_for(n), dim3(256), 0, ctx.stream, __VA_ARGS__);            \
    MAA_HIP(hipGetLastError())
