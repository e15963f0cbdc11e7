// MX-FP8 (OCP e4m3fn elements, one E8M0 scale per 32 consecutive K elements): the ONE definition of the quantiser,
// shared by vc_mx8_quantize (bank input, weight packing) and the epilogue of mx8_conv_kernel (bank output), so the two
// cannot drift apart.  tests/mx8_ref.py is the CPU statement of the same rule, written independently (code table).
//
// Scale rule: e is the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127]; the E8M0 code is e + 127.
// The block's largest element therefore scales into (224, 448] and nothing saturates.  Elements are RNE(x * 2^-e) in
// e4m3fn with subnormals kept; the sign bit is x's (a negative value that rounds to zero is 0x80).  A block whose amax
// is zero gets scale code 0 and zero (0x00) elements.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vc {

// exponent e of the block scale (see above); amax > 0, finite
__device__ __forceinline__ int mx8_scale_exp(float amax) {
    uint32_t b = __float_as_uint(amax);
    int bias_e = (int)(b >> 23);
    if (bias_e == 0) {                                   // f32 subnormal: normalise exactly
        b = __float_as_uint(amax * 16777216.0f);         // * 2^24
        bias_e = (int)(b >> 23) - 24;
    }
    // amax = 1.m * 2^(bias_e - 127); 448 = 1.75 * 2^8: mantissa <= 1.75 -> e = ea - 8, else ea - 7
    const int e = bias_e - 127 - 8 + ((b & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    return min(max(e, -127), 127);
}

// e4m3fn code of RNE(x * 2^-e); |x * 2^-e| <= 448 by the scale rule
__device__ __forceinline__ uint32_t mx8_encode(float x, int e) {
    const float v = fabsf(ldexpf(x, -e));
    const uint32_t sign = (__float_as_uint(x) >> 24) & 0x80u;
    uint32_t code;
    if (v < 0.015625f) {                                 // below 2^-6: subnormal codes m * 2^-9 (8 -> smallest normal)
        code = (uint32_t)rintf(v * 512.0f);
    } else {                                             // round the f32 mantissa to 3 bits, ties to even; rebias 127 -> 7
        const uint32_t b = __float_as_uint(v);
        code = ((b + 0x7FFFFu + ((b >> 20) & 1u)) >> 20) - (120u << 3);
    }
    return code | sign;
}

}  // namespace vc
