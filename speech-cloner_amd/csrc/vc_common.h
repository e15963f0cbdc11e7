// Shared host/device helpers for libvc_hip.so (error reporting, wave/block reductions).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include "vc_hip.h"

namespace vc {

char* last_error_buf();
int set_error(int code, const char* fmt, ...);

#define VC_HIP_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return vc::set_error(VC_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                 \
                                 hipGetErrorString(_e), __FILE__, __LINE__);                 \
    } while (0)

#define VC_REQUIRE(cond, ...)                                                                \
    do {                                                                                     \
        if (!(cond)) return vc::set_error(VC_ERR_INVALID, __VA_ARGS__);                      \
    } while (0)

constexpr int WAVE = 64;

// Kernel-selection options (vc_set_option / vc_get_option, include/vc_hip.h).  -1 = the library's own choice.
// They pick between HIP kernels that compute the SAME function (A/B measurements, regression tests); nothing in
// the library reads the process environment, and no option changes what a kernel computes.
enum Option {
    OPT_BANK256 = 0,      // 0: filter banks on conv_kernel instead of bank256_kernel
    OPT_BANK256_XCD,      // 0: plain 2-D grid, 1: whole pairs per XCD, 2: pairs split over two XCDs (default)
    OPT_CONV256,          // 0: long-K single filters on conv_kernel / gemm_kernel instead of conv256_kernel
    OPT_CONV256_MINK,     // shortest K that takes conv256_kernel (default 384)
    OPT_CONV256_WM,       // 2: keep 128-row blocks for 128-column launches (default: 256 rows from 2,048 rows up)
    OPT_PROJ256,          // 0: 256-channel long-K projection on conv256_kernel instead of the bank tiles
    OPT_PROJ256_SPLIT,    // 0: never split that projection's K over two workgroups per row tile
    OPT_WGRAD_XCD,        // 0: weight-gradient tiles dealt round-robin instead of group-per-XCD
    OPT_GRU_MFMA,         // 0: VALU recurrence always, 1: MFMA recurrence always (default: vc_gru_bidir from 32 sequences up, vc_gru_form by makespan)
    OPT_FE_FUSED,         // 0: the shipped front-end configuration as two launches (statistics pass + feature pass) instead of one
    OPT_FE_FUSED_SPIN,    // polls a block of the one-launch front-end waits for its utterance's tiles (default 4000 ~ 4 ms); 0: never wait
    OPT_PRENET_LDS,       // 0: every wave of prenet_chain streams the weights itself (default: shared through LDS)
    OPT_GRU_TRAIN_RESIDENT,   // 0: the float32 training recurrences stream all their weights from L2 every step
    OPT_CBHG_FRONT_MI,    // 4: 128-row blocks in cbhg_small_kernel (default 2)
    OPT_GRU_F32_WIDE,     // 0: float32 inference recurrences of more than 128 units stay on gru_generic_kernel (default: the training forward kernel)
    OPT_F32_F16X3,        // 0: float32 inference convolutions stay on the f32-input MFMA kernels (default: vc_gemm16)
    OPT_GEMM16_SPLIT,     // vc_gemm16 single-pair launches: K split ways (1..8) + 16 * block map (0: a row tile's splits on one XCD, 1: a K range per XCD); default: automatic
    OPT_COUNT
};
int opt(Option o);        // current value, -1 if unset

// Zeroes `bytes` (a multiple of 4) at d_p with a kernel on `st`.  Every per-launch word that a kernel polls or
// accumulates into is cleared this way and not with hipMemsetAsync: under graph capture a memset node of the HIP
// runtime this library is built against cleared only three quarters of its bytes from the second replay on
// (tests/test_graph_replay_gpu.py), while a kernel node is replayed like any other launch.
hipError_t zero_async(void* d_p, size_t bytes, hipStream_t st);

#if defined(__HIPCC__)
// Wave-wide reductions on DPP (data-parallel primitives: the cross-lane operand of a VALU instruction), result in every
// lane.  __shfl_xor lowers to ds_bpermute_b32 on gfx950 -- an LDS-path round trip of ~100 cycles per step, 6 dependent
// steps per reduction; the DPP form is 6 plain vector instructions (quad swaps, half-row / row mirrors, then the
// row_bcast:15 / row_bcast:31 carries of the GFX9 family) and one v_readlane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float identity, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
#define VC_WAVE_REDUCE(OP, ID)                                                                  \
    v = OP(v, dpp_move<0xB1, 0xF>(ID, v));     /* quad_perm [1,0,3,2] */                        \
    v = OP(v, dpp_move<0x4E, 0xF>(ID, v));     /* quad_perm [2,3,0,1] */                        \
    v = OP(v, dpp_move<0x141, 0xF>(ID, v));    /* row_half_mirror */                            \
    v = OP(v, dpp_move<0x140, 0xF>(ID, v));    /* row_mirror: every lane of a row of 16 */      \
    v = OP(v, dpp_move<0x142, 0xA>(ID, v));    /* row_bcast:15 into rows 1 and 3 */             \
    v = OP(v, dpp_move<0x143, 0xC>(ID, v));    /* row_bcast:31 into rows 2 and 3 */             \
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
__device__ __forceinline__ float vc_addf(float a, float b) { return a + b; }
__device__ __forceinline__ float wave_sum(float v) { VC_WAVE_REDUCE(vc_addf, 0.0f) }
// wave_max / wave_min are for FINITE data: a lane whose source a step disables takes the seed, +-FLT_MAX, so a wave that
// holds nothing but -inf (+inf) comes back as the seed.  wave_max_inf seeds every step with the lane's own value and so
// keeps an all -inf wave at -inf (the log-domain rows of vc_fullsum.hip).
__device__ __forceinline__ float wave_max(float v) { VC_WAVE_REDUCE(fmaxf, -3.402823466e38f) }
__device__ __forceinline__ float wave_max_inf(float v) { VC_WAVE_REDUCE(fmaxf, v) }
// highwaynet gate (modules.py:315-319): relu(h) * t + x * (1 - t), t = sigmoid(tpre), written as
// x + t * (relu(h) - x) with v_exp_f32 / v_rcp_f32 (1 ulp each) -- the gate arithmetic, not the
// matrix work, bounds the fused highway chain, and an IEEE division costs ~10 instructions.
// gemm_kernel's highway epilogue and highway_chain_kernel share it (bit-identical paths).
__device__ __forceinline__ float highway_gate(float hpre, float tpre, float x) {
    const float hv = fmaxf(hpre, 0.0f);
    const float e = __builtin_amdgcn_exp2f(tpre * -1.4426950408889634f);
    const float tv = __builtin_amdgcn_rcpf(1.0f + e);
    return fmaf(tv, hv - x, x);
}
__device__ __forceinline__ float wave_min(float v) { VC_WAVE_REDUCE(fminf, 3.402823466e38f) }
#undef VC_WAVE_REDUCE
// The greatest value over the wave and its index, the lowest index where several lanes hold that value; in every lane.
struct ArgMax { float v; int idx; };
__device__ __forceinline__ ArgMax wave_argmax_low(float v, int idx) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float ov = __shfl_xor(v, s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    return {v, idx};
}

// Exclusive scans over a workgroup of NW waves: the value of the lanes before this one combined (the identity for lane
// 0: 0 for the sum, -1 for the maximum) and, in `total`, of all lanes.  Inside a wave by shuffles, the waves' totals
// through wtot[NW] in LDS; two barriers a scan, every lane of the workgroup must call it.
template <bool SUM, int NW>
__device__ inline int block_scan_excl(int v, int* wtot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ident = SUM ? 0 : -1;
    int inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int u = __shfl_up(inc, s, 64);
        if (lane >= s) inc = SUM ? inc + u : max(inc, u);
    }
    int excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = ident;
    __syncthreads();                                                // the previous scan's reads of wtot
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int off = ident, all = ident;
    for (int w = 0; w < NW; ++w) {
        const int x = wtot[w];
        if (w < wave) off = SUM ? off + x : max(off, x);
        all = SUM ? all + x : max(all, x);
    }
    total = all;
    return SUM ? excl + off : max(excl, off);
}

// The vocoder's magnitude of one normalised power value in dB (audio_lib.py:289-298 with realse == 1):
// sqrt(db_to_power(max(0, P) / norm - 80)).  vc_compound_stitch and vc_time_warp fuse it; vc_power_to_amp's kernel
// (vc_vocoder.hip) evaluates the same expression after its optional power law.
__device__ __forceinline__ float power_db_to_amp(float P, float inv_norm) {
    return exp10f(0.05f * (fmaxf(0.0f, P) * inv_norm - 80.0f));
}
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): vc_phase_init and vc_noise_init_f32 address it alike.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
#endif

}  // namespace vc
