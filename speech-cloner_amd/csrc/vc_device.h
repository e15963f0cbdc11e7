// Device helpers shared by the tile kernels: vector types, the LDS-direct load, the post-ReLU pool maximum, epilogue
// activations, the SAME-padding tap range of a row and of a wave, workspace alignment, and the once-per-kernel
// dynamic-LDS opt-in of the launchers.  Each is defined here once; a .hip file keeps only what is its own.
#pragma once
#include <cstdint>
#include "vc_common.h"

namespace vc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// workspace sections start on 256-byte boundaries
__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Raises the dynamic-LDS limit of the given kernels to `bytes`, once per process: every distinct kernel list is its own
// instantiation with its own flag.  One call per launch site: `if (int rc = vc::allow_dynamic_lds<kernel>(bytes)) return rc;`
template <auto... Kernels>
int allow_dynamic_lds(int bytes) {
    static bool done = false;
    if (!done) {
        for (const void* k : {reinterpret_cast<const void*>(Kernels)...})
            VC_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        done = true;
    }
    return VC_OK;
}

// global_load_lds, 16 bytes per lane: global address g straight into LDS address l (no register hop)
__device__ __forceinline__ void glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(uintptr_t)g,
                                     (__attribute__((address_space(3))) void*)(uintptr_t)(uint32_t)(uintptr_t)l, 16, 0, 0);
}

// XOR key of the 16-byte slot of row r in a 128-byte-row LDS tile whose fragments feed v_mfma_f32_16x16x32_bf16 (lane l reads row
// l & 15, slot (l >> 4) + 4 * step): every ds_read_b128 is conflict-free at any row offset (worked out in vc_bank256.hip).
__device__ __forceinline__ int slot_key16(int r) { return ((r >> 1) & 3) << 1; }

// max of values that are >= 0 (post-ReLU), either zero included: for them IEEE ordering == SIGNED integer ordering
// of the bit patterns (-0.0 is the most negative integer, so it loses to every other such value, where the
// unsigned order would rank it above all of them), so bf16 pairs go through v_pk_max_i16 and f32 through v_max_i32.
__device__ __forceinline__ bf16x8 max_nonneg(bf16x8 a, bf16x8 b) {
    const i16x8 r = __builtin_elementwise_max(__builtin_bit_cast(i16x8, a), __builtin_bit_cast(i16x8, b));
    return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ f32x4 max_nonneg(f32x4 a, f32x4 b) {
    const i32x4 r = __builtin_elementwise_max(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b));
    return __builtin_bit_cast(f32x4, r);
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }

__device__ __forceinline__ float act_fn(float v, int act) {
    switch (act) {
        case VC_ACT_RELU: return fmaxf(v, 0.0f);
        case VC_ACT_SIGMOID: return 1.0f / (1.0f + __expf(-v));
        case VC_ACT_TANH: return tanhf(v);
        default: return v;
    }
}

// SAME padding per window of T frames: the row at global frame m (frame t = m % T of its window) reads a real frame at
// taps [jlo, jhi) of a filter with pad_l taps of left padding; the other taps fall outside the window and contribute 0.
__device__ __forceinline__ void same_tap_range(int m, int T, int pad_l, int& jlo, int& jhi) {
    const int t = m % T;
    jlo = max(0, pad_l - t);
    jhi = T - t + pad_l;
}
// The range that holds for every lane of the wave (largest lo, smallest hi), made provably wave-uniform so that the
// per-tile test on it is a scalar branch.
__device__ __forceinline__ void wave_tap_range(int& J_lo, int& J_hi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        J_lo = max(J_lo, __shfl_xor(J_lo, o, 64));
        J_hi = min(J_hi, __shfl_xor(J_hi, o, 64));
    }
    J_lo = __builtin_amdgcn_readfirstlane(J_lo);
    J_hi = __builtin_amdgcn_readfirstlane(J_hi);
}

}  // namespace vc
