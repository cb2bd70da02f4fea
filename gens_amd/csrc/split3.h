// Three-term bf16 operands of the float32-accurate bf16 MFMA kernels (k6b_sdf_bf16x3.hip, k7b_blend_bf16x3.hip): every float32 value is
// x = x0 + x1 + x2, three round-to-nearest bf16 terms; the residuals x - x0 and x - x0 - x1 are exact in float32, so the three terms carry
// all 24 bits of the significand at float32's exponent range.
#pragma once
#include <stdint.h>

typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define SPLIT3_TERMS 3

struct Split3Block {      // one lane's 8 K slots of a bf16 MFMA operand as three bf16 terms
    u32x4 p[SPLIT3_TERMS];
};

struct Split3Word {
    uint32_t w[SPLIT3_TERMS];
};
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {      // v_cvt_pk_bf16_f32: a -> bits [15:0], b -> [31:16], nearest even
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2v){a, b}, bf16x2));
}
// (a, b) -> their three packed terms; the residuals a - x0, a - x0 - x1 are exact in float32.  PACKED: the two residuals of a step in one
// v_pk_add_f32 (the same values; for kernels whose vector pipe is the busy one)
template <bool PACKED = false>
__device__ __forceinline__ Split3Word split3_pair(float a, float b) {
    Split3Word s;
#pragma unroll
    for (int k = 0; k < SPLIT3_TERMS; ++k) {
        const uint32_t w = pk_bf16(a, b);
        s.w[k] = w;
        if (k + 1 < SPLIT3_TERMS) {
            if (PACKED) {
                const f32x2v r = (f32x2v){a, b} - (f32x2v){__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
                a = r[0];
                b = r[1];
            } else {
                a -= __builtin_bit_cast(float, w << 16);
                b -= __builtin_bit_cast(float, w & 0xffff0000u);
            }
        }
    }
    return s;
}
