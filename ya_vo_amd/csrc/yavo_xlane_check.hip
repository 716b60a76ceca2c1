// yavo_xlane_check.hip -- yavo_xlane.h self-check (tests/test_gpu_xlane.py): rows 0-3 = lane ^ {1, 2, 4, 8} through the
// DPP butterflies; rows 4-5 / 6-7 = the permlane16 / permlane32 half exchange of (lo = lane, hi = 100 + lane).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yavo_xlane.h"

namespace yavo {
__global__ void xlane_check_kernel(int32_t* out) {
    const int l = threadIdx.x;
    out[0 * 64 + l] = xl::xor_row_i32<1>(l);
    out[1 * 64 + l] = xl::xor_row_i32<2>(l);
    out[2 * 64 + l] = xl::xor_row_i32<4>(l);
    out[3 * 64 + l] = xl::xor_row_i32<8>(l);
    uint32_t a = (uint32_t)l, b = 100u + (uint32_t)l;
    xl::swap_halves<16>(a, b);
    out[4 * 64 + l] = (int32_t)a;
    out[5 * 64 + l] = (int32_t)b;
    a = (uint32_t)l;
    b = 100u + (uint32_t)l;
    xl::swap_halves<32>(a, b);
    out[6 * 64 + l] = (int32_t)a;
    out[7 * 64 + l] = (int32_t)b;
}
}  // namespace yavo

extern "C" int yv_debug_xlane(int32_t* d_out /* [8][64] */, void* stream) {
    if (!d_out) return -1;
    hipLaunchKernelGGL(yavo::xlane_check_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), d_out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
