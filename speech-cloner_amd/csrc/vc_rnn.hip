// Recurrent + row-wise kernels of the network path (contract: include/vc_hip.h):
//   vc_gru_bidir       bidirectional GRU recurrence (/root/reference/modules.py:168-204)
//   vc_softmax_argmax  tf.nn.softmax + tf.argmax (/root/reference/encoder.py:110-111)
//   vc_convert         f32 <-> bf16
//
// GRU: the time loop is strictly serial (400 steps per direction), so one workgroup owns one
// (window, direction) pair for the whole sequence: h never leaves the CU (LDS), the recurrent
// weights stay on chip whenever they fit (LDS here; registers in gru_resident below) and only the
// hoisted input projections stream in (prefetched one step ahead).  No cross-CU exchange per
// step -- that costs >= 1 us on this chip (MI355X_MICROARCH.md, hand-off price list), more than a
// whole step.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdlib>

#include "vc_device.h"

using vc::f32x4, vc::bf16x8, vc::bf16x4, vc::bf16x2;

namespace {

__device__ __forceinline__ float ld_w(const float* p) { return *p; }
__device__ __forceinline__ float ld_w(const __bf16* p) { return (float)*p; }
// bf16 recurrences: v_exp_f32 + v_rcp_f32 (1 ulp each) instead of libm tanhf / IEEE division --
// the gate arithmetic of 16 sequences lands on one CU in the MFMA kernel, so it must be cheap.
__device__ __forceinline__ float fast_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
__device__ __forceinline__ float fast_tanh(float v) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * v) + 1.0f); }

struct GruArgs {
    const float* xproj;     // [n_seq*T, 6H]
    const void* Wh[2];      // [H, 3H] per direction
    void* out;              // [n_seq*T, 2H]
    int32_t n_seq, T, H, out_bf16, w_in_lds;
};

template <typename T> __device__ __forceinline__ void st_out(void* o, size_t i, float v, int bf) {
    if (bf) reinterpret_cast<__bf16*>(o)[i] = (__bf16)v;
    else reinterpret_cast<float*>(o)[i] = v;
}

// Generic recurrence: any H <= 1024.  Thread group (col, ks): column `col` of the phase's weight block, K-slice
// ks of KS (KS a power of two <= 64, lanes of one column adjacent => shuffle reduction).  NT / KS groups exist; a group
// takes columns col, col + NT / KS, ...: one column per group up to H = 256 (2H <= NT = 512), up to GEN_C1 gate and
// GEN_C2 candidate columns per thread beyond (KS = 1 there).
constexpr int GEN_NT_MAX = 512, GEN_H_MAX = 1024;
constexpr int GEN_C1 = 2 * GEN_H_MAX / GEN_NT_MAX, GEN_C2 = GEN_H_MAX / GEN_NT_MAX;
template <typename WT>
__global__ void __launch_bounds__(GEN_NT_MAX)
gru_generic_kernel(GruArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, H3 = 3 * H, NT = blockDim.x, tid = threadIdx.x;
    float* h = reinterpret_cast<float*>(smem);      // [H]
    float* rh = h + H;                              // [H]
    float* u = rh + H;                              // [H]
    WT* wl = reinterpret_cast<WT*>(u + H);          // [H][3H] when cached
    const int seq = blockIdx.x, dir = blockIdx.y;
    const WT* Wg = reinterpret_cast<const WT*>(a.Wh[dir]);
    if (a.w_in_lds) {
        for (int i = tid; i < H * H3; i += NT) wl[i] = Wg[i];
        Wg = wl;
    }
    for (int i = tid; i < H; i += NT) h[i] = 0.0f;

    int KS1 = 1, KS2 = 1;
    while (KS1 * 2 <= 64 && KS1 * 2 * 2 * H <= NT) KS1 *= 2;
    while (KS2 * 2 <= 64 && KS2 * 2 * H <= NT) KS2 *= 2;
    const int col1 = tid / KS1, ks1 = tid % KS1, cs1 = NT / KS1;      // gate columns col1 + i cs1 in [0, 2H)
    const int col2 = tid / KS2, ks2 = tid % KS2, cs2 = NT / KS2;      // candidate columns col2 + i cs2 in [0, H)
    const size_t xrow = 6 * (size_t)H;
    const float* xbase = a.xproj + (size_t)seq * a.T * xrow + (size_t)dir * H3;
    __syncthreads();

    int t = dir ? a.T - 1 : 0;
    const int dt = dir ? -1 : 1;
    float xg[GEN_C1], xc[GEN_C2];
#pragma unroll
    for (int i = 0; i < GEN_C1; ++i) {
        const int col = col1 + i * cs1;
        xg[i] = (col < 2 * H && ks1 == 0) ? xbase[(size_t)t * xrow + col] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < GEN_C2; ++i) {
        const int col = col2 + i * cs2;
        xc[i] = (col < H && ks2 == 0) ? xbase[(size_t)t * xrow + 2 * H + col] : 0.0f;
    }
    for (int step = 0; step < a.T; ++step, t += dt) {
        // prefetch next step's input projections
        float xg_n[GEN_C1], xc_n[GEN_C2];
        const bool more = step + 1 < a.T;
#pragma unroll
        for (int i = 0; i < GEN_C1; ++i) {
            const int col = col1 + i * cs1;
            xg_n[i] = (more && col < 2 * H && ks1 == 0) ? xbase[(size_t)(t + dt) * xrow + col] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < GEN_C2; ++i) {
            const int col = col2 + i * cs2;
            xc_n[i] = (more && col < H && ks2 == 0) ? xbase[(size_t)(t + dt) * xrow + 2 * H + col] : 0.0f;
        }
        // phase 1: gates (a column's KS1 lanes take the branch together)
#pragma unroll
        for (int i = 0; i < GEN_C1; ++i) {
            const int col = col1 + i * cs1;
            if (col >= 2 * H) break;
            float acc = 0.0f;
            const WT* w = Wg + col;
            for (int k = ks1; k < H; k += KS1) acc = fmaf(h[k], ld_w(w + (size_t)k * H3), acc);
            for (int o = KS1 >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (ks1 == 0) {
                const float g = vc::sigmoidf_(acc + xg[i]);
                if (col < H) rh[col] = g * h[col];          // r first (GRUCell split order)
                else u[col - H] = g;
            }
        }
        __syncthreads();
        // phase 2: candidate
        float hn[GEN_C2];
#pragma unroll
        for (int i = 0; i < GEN_C2; ++i) {
            const int col = col2 + i * cs2;
            hn[i] = 0.0f;
            if (col >= H) break;
            float acc2 = 0.0f;
            const WT* w = Wg + 2 * H + col;
            for (int k = ks2; k < H; k += KS2) acc2 = fmaf(rh[k], ld_w(w + (size_t)k * H3), acc2);
            for (int o = KS2 >> 1; o > 0; o >>= 1) acc2 += __shfl_xor(acc2, o, 64);
            if (ks2 == 0) {
                const float c = tanhf(acc2 + xc[i]);
                const float uu = u[col];
                hn[i] = uu * h[col] + (1.0f - uu) * c;
            }
        }
        __syncthreads();                                // everyone done reading h / rh
#pragma unroll
        for (int i = 0; i < GEN_C2; ++i) {
            const int col = col2 + i * cs2;
            if (col < H && ks2 == 0) {
                h[col] = hn[i];
                st_out<WT>(a.out, ((size_t)seq * a.T + t) * 2 * H + (size_t)dir * H + col, hn[i], a.out_bf16);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GEN_C1; ++i) xg[i] = xg_n[i];
#pragma unroll
        for (int i = 0; i < GEN_C2; ++i) xc[i] = xc_n[i];
    }
}


// ------------------------------------------------------------------------------------------
// LSTM recurrence (modules.py:207-243 -> tf.contrib.rnn.LSTMCell, no peepholes, no projection, forget_bias 1.0):
//   z = [x, h] W + b;  i, j, f, o = split(z, 4);  c' = sigmoid(f + 1) c + sigmoid(i) tanh(j);  h' = sigmoid(o) tanh(c')
// xproj [n_seq*T, 8H] float32 holds x W_x + b of both directions (fw | bw, 4H each); Wh[dir] is the recurrent half
// [H, 4H].  One workgroup per (sequence, direction); a thread owns gate columns tid, tid + NT, ...  No shipped
// configuration enables use_lstm: a plain, any-H kernel (weights from LDS when they fit, else L2), not a tuned one.
struct LstmArgs {
    const float* xproj;
    const void* Wh[2];
    int32_t n_seq, T, H;
    void* out;
    int32_t out_bf16, w_in_lds;
};

template <typename WT>
__global__ void __launch_bounds__(512)
lstm_generic_kernel(LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, H4 = 4 * H, NT = blockDim.x, tid = threadIdx.x;
    float* h = reinterpret_cast<float*>(smem);      // [H]
    float* z = h + H;                               // [4H]
    WT* wl = reinterpret_cast<WT*>(z + H4);         // [H][4H] when cached
    const int seq = blockIdx.x, dir = blockIdx.y;
    const WT* W = reinterpret_cast<const WT*>(a.Wh[dir]);
    if (a.w_in_lds) {
        for (int i = tid; i < H * H4; i += NT) wl[i] = W[i];
        W = wl;
    }
    for (int i = tid; i < H; i += NT) h[i] = 0.0f;
    float c = 0.0f;                                 // cell state of unit tid (threads tid < H; H <= NT asserted by the host)
    const size_t xrow = 8 * (size_t)H;
    const float* xbase = a.xproj + (size_t)seq * a.T * xrow + (size_t)dir * H4;
    __syncthreads();
    int t = dir ? a.T - 1 : 0;
    const int dt = dir ? -1 : 1;
    for (int step = 0; step < a.T; ++step, t += dt) {
        const float* xr = xbase + (size_t)t * xrow;
        for (int col = tid; col < H4; col += NT) {
            float acc = xr[col];
            const WT* w = W + col;
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(h[k], ld_w(w + (size_t)k * H4), acc);
            z[col] = acc;
        }
        __syncthreads();
        if (tid < H) {
            const float gi = vc::sigmoidf_(z[tid]), gj = tanhf(z[H + tid]);
            const float gf = vc::sigmoidf_(z[2 * H + tid] + 1.0f), go = vc::sigmoidf_(z[3 * H + tid]);
            c = gf * c + gi * gj;
            const float hn = go * tanhf(c);
            h[tid] = hn;
            st_out<WT>(a.out, ((size_t)seq * a.T + t) * 2 * H + (size_t)dir * H + tid, hn, a.out_bf16);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Register-resident recurrence (H = 128 or 256): NT threads hold the WHOLE recurrent matrix
// [H, 3H] in VGPRs for all T steps (bf16 at H = 256: 3H^2*2 B = 393 KB of the CU's 512 KB register
// file = 192 VGPRs per lane at NT = 512, two waves per SIMD; H = 128: NT = 1024, 24 (bf16) or 48
// (f32) VGPRs per lane).  Per step only h (LDS, bf16
// copy for v_dot2c_f32_bf16 + f32 copy for the gate arithmetic) and one prefetched row of the
// hoisted input projections move.
//   phase 1: thread (col1 = tid / KS1, ks1 = tid % KS1) owns K-slice ks1 of gate column col1 (2H
//            columns), KS1 = NT / 2H adjacent lanes are summed with DPP-style shuffles;
//   phase 2: thread (col2 = tid / KS2, ks2) the same for the H candidate columns, KS2 = NT / H.
// Two barriers per step; h_old of a column lives in the owning thread's register.

// Weights arrive PRE-PACKED by gru_pack_kernel in the exact register order:
//   packed[dir][chunk c][thread tid][EPC elements]  (one 16-byte chunk per lane => coalesced)
// chunk c of thread tid covers elements j = c*EPC .. c*EPC+EPC-1 of its concatenated slices
// [phase-1 slice (KL1) | phase-2 slice (KL2)], so the preload is (KL1+KL2)/EPC direct 16-B loads.
template <typename WT> struct Res;
template <> struct Res<__bf16> {
    static constexpr int EPC = 8;                            // elements per 16-byte chunk
    typedef __bf16 hstore_t;
    typedef bf16x8 chunk_t;
    static __device__ __forceinline__ void dot(const chunk_t& w, const __bf16* hs, float& a0, float& a1) {
        const bf16x8 hv = *reinterpret_cast<const bf16x8*>(hs);
        const bf16x2 w0 = {w[0], w[1]}, w1 = {w[2], w[3]}, w2 = {w[4], w[5]}, w3 = {w[6], w[7]};
        const bf16x2 h0 = {hv[0], hv[1]}, h1 = {hv[2], hv[3]}, h2 = {hv[4], hv[5]}, h3 = {hv[6], hv[7]};
        a0 = __builtin_amdgcn_fdot2_f32_bf16(w0, h0, a0, false);
        a1 = __builtin_amdgcn_fdot2_f32_bf16(w1, h1, a1, false);
        a0 = __builtin_amdgcn_fdot2_f32_bf16(w2, h2, a0, false);
        a1 = __builtin_amdgcn_fdot2_f32_bf16(w3, h3, a1, false);
    }
};
template <> struct Res<float> {
    static constexpr int EPC = 4;
    typedef float hstore_t;
    typedef f32x4 chunk_t;
    static __device__ __forceinline__ void dot(const chunk_t& w, const float* hs, float& a0, float& a1) {
        const f32x4 hv = *reinterpret_cast<const f32x4*>(hs);
        a0 = fmaf(w[0], hv[0], a0);
        a1 = fmaf(w[1], hv[1], a1);
        a0 = fmaf(w[2], hv[2], a0);
        a1 = fmaf(w[3], hv[3], a1);
    }
};

template <int H, int NT> struct ResGeom {
    static constexpr int KS1 = NT / (2 * H), KL1 = H / KS1, KS2 = NT / H, KL2 = H / KS2;
};

// [H, 3H] row-major -> packed register order (see above); one launch handles both directions.
template <int H, typename WT, int NT>
__global__ void __launch_bounds__(256)
gru_pack_kernel(const WT* W0, const WT* W1, WT* packed) {
    typedef ResGeom<H, NT> G;
    constexpr int EPC = Res<WT>::EPC, PER = G::KL1 + G::KL2, H3 = 3 * H;
    const int total = 2 * NT * PER;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int dir = idx / (NT * PER);
        int r = idx - dir * NT * PER;
        const int c = r / (NT * EPC);
        r -= c * NT * EPC;
        const int tid = r / EPC, e = r - tid * EPC;
        const int j = c * EPC + e;
        const WT* W = dir ? W1 : W0;
        WT v;
        if (j < G::KL1) {
            const int col1 = tid / G::KS1, ks1 = tid % G::KS1;
            v = W[(size_t)(ks1 * G::KL1 + j) * H3 + col1];
        } else {
            const int col2 = tid / G::KS2, ks2 = tid % G::KS2;
            v = W[(size_t)(ks2 * G::KL2 + (j - G::KL1)) * H3 + 2 * H + col2];
        }
        packed[idx] = v;
    }
}

template <int H, typename WT, int NT>
__global__ void __launch_bounds__(NT, NT / 256)
gru_resident_kernel(GruArgs a, const WT* packed) {
    typedef Res<WT> R;
    typedef ResGeom<H, NT> G;
    typedef typename R::hstore_t hs_t;
    typedef typename R::chunk_t chunk_t;
    constexpr int H3 = 3 * H, EPC = R::EPC;
    constexpr int KS1 = G::KS1, KL1 = G::KL1, KS2 = G::KS2, KL2 = G::KL2;
    constexpr int NC1 = KL1 / EPC, NC2 = KL2 / EPC;
    constexpr int P = EPC;                                   // 16-byte pad between K-slices
    static_assert(KS1 >= 1 && KS2 <= 64 && KL1 % EPC == 0 && KL2 % EPC == 0, "unsupported H");
    static_assert(2 * H <= NT, "one thread per gate column at least");
    __shared__ __attribute__((aligned(16))) hs_t hb[KS1 * (KL1 + P)];     // h, sliced for phase 1
    __shared__ __attribute__((aligned(16))) hs_t rhb[KS2 * (KL2 + P)];    // r*h, sliced for phase 2
    __shared__ float hf[H];                                               // h in f32 (for r*h)
    __shared__ float ul[H];                                               // update gate

    const int tid = threadIdx.x;
    const int seq = blockIdx.x, dir = blockIdx.y;
    const int col1 = tid / KS1, ks1 = tid % KS1;
    const int col2 = tid / KS2, ks2 = tid % KS2;
    chunk_t w1[NC1], w2[NC2];
    {
        const chunk_t* pk = reinterpret_cast<const chunk_t*>(packed) + (size_t)dir * NT * (NC1 + NC2) + tid;
#pragma unroll
        for (int c = 0; c < NC1; ++c) w1[c] = pk[(size_t)c * NT];
#pragma unroll
        for (int c = 0; c < NC2; ++c) w2[c] = pk[(size_t)(NC1 + c) * NT];
    }
    for (int i = tid; i < KS1 * (KL1 + P); i += NT) hb[i] = (hs_t)0.0f;
    for (int i = tid; i < KS2 * (KL2 + P); i += NT) rhb[i] = (hs_t)0.0f;
    if (tid < H) hf[tid] = 0.0f;
    const size_t xrow = 6 * (size_t)H;
    const float* xbase = a.xproj + (size_t)seq * a.T * xrow + (size_t)dir * H3;
    int t = dir ? a.T - 1 : 0;
    const int dt = dir ? -1 : 1;
    float xg = (ks1 == 0) ? xbase[(size_t)t * xrow + col1] : 0.0f;
    float xc = (ks2 == 0) ? xbase[(size_t)t * xrow + 2 * H + col2] : 0.0f;
    float hreg = 0.0f;
    const hs_t* hs1 = hb + ks1 * (KL1 + P);
    const hs_t* hs2 = rhb + ks2 * (KL2 + P);
    __syncthreads();

    for (int step = 0; step < a.T; ++step, t += dt) {
        float xg_n = 0.0f, xc_n = 0.0f;
        if (step + 1 < a.T) {
            if (ks1 == 0) xg_n = xbase[(size_t)(t + dt) * xrow + col1];
            if (ks2 == 0) xc_n = xbase[(size_t)(t + dt) * xrow + 2 * H + col2];
        }
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int c = 0; c < NC1; ++c) R::dot(w1[c], hs1 + c * EPC, a0, a1);
        float acc = a0 + a1;
#pragma unroll
        for (int o = KS1 >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (ks1 == 0) {
            const float g = (sizeof(WT) == 2) ? fast_sigmoid(acc + xg) : vc::sigmoidf_(acc + xg);
            if (col1 < H) {
                const int s = col1 / KL2, off = col1 - s * KL2;
                rhb[s * (KL2 + P) + off] = (hs_t)(g * hf[col1]);
            } else {
                ul[col1 - H] = g;
            }
        }
        __syncthreads();
        float b0 = 0.0f, b1 = 0.0f;
#pragma unroll
        for (int c = 0; c < NC2; ++c) R::dot(w2[c], hs2 + c * EPC, b0, b1);
        float acc2 = b0 + b1;
#pragma unroll
        for (int o = KS2 >> 1; o > 0; o >>= 1) acc2 += __shfl_xor(acc2, o, 64);
        if (ks2 == 0) {
            const float c = (sizeof(WT) == 2) ? fast_tanh(acc2 + xc) : tanhf(acc2 + xc);
            const float uu = ul[col2];
            const float hn = uu * hreg + (1.0f - uu) * c;
            hreg = hn;
            const int s = col2 / KL1, off = col2 - s * KL1;
            hb[s * (KL1 + P) + off] = (hs_t)hn;
            hf[col2] = hn;
            st_out<WT>(a.out, ((size_t)seq * a.T + t) * 2 * H + (size_t)dir * H + col2, hn, a.out_bf16);
        }
        __syncthreads();
        xg = xg_n;
        xc = xc_n;
    }
}

// Packing and running are separate launches: the packed image depends on the weights alone, so a caller whose weights
// stay put packs once (vc_gru_pack) and runs on the image (vc_gru_bidir_packed); vc_gru_bidir packs into its workspace
// on every call.
template <int H, typename WT, int NT>
void pack_resident(const void* Wfw, const void* Wbw, void* packed, hipStream_t st) {
    hipLaunchKernelGGL((gru_pack_kernel<H, WT, NT>), dim3(256), dim3(256), 0, st, static_cast<const WT*>(Wfw),
                       static_cast<const WT*>(Wbw), static_cast<WT*>(packed));
}

template <int H, typename WT, int NT>
int run_resident(const GruArgs& a, const void* packed, hipStream_t st) {
    hipLaunchKernelGGL((gru_resident_kernel<H, WT, NT>), dim3(a.n_seq, 2), dim3(NT), 0, st, a,
                       static_cast<const WT*>(packed));
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

template <int H, typename WT, int NT>
int launch_resident(const GruArgs& a, void* ws, size_t ws_bytes, hipStream_t st) {
    const size_t need = 2 * (size_t)3 * H * H * sizeof(WT);
    if (ws == nullptr || ws_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_gru_bidir: workspace too small (%zu < %zu)", ws_bytes, need);
    pack_resident<H, WT, NT>(a.Wh[0], a.Wh[1], ws, st);
    return run_resident<H, WT, NT>(a, ws, st);
}


// ------------------------------------------------------------------------------------------
// MFMA recurrence (bf16, H = 128 / 256): ONE workgroup advances 16 sequences of one direction.
//   v_mfma_f32_16x16x32_bf16:  D[unit i][seq n] += A[unit i][k] * B[k][seq n]
//   A = transposed recurrent weights (tile of 16 hidden units x 32 k), resident for all T steps:
//       gate (r,u) tiles in VGPRs, candidate tiles in VGPRs (H = 128) or LDS (H = 256: 128 KB);
//   B = the 16 hidden-state vectors (bf16, LDS, one ds_read_b128 per lane and k-step).
// Wave w owns hidden units [w*H/8, (w+1)*H/8): its r, u and c accumulators for a (unit, sequence)
// pair live in the same lane and register, so the whole gate arithmetic is lane-local; only r*h
// and h cross waves (LDS, two barriers per step).  The matrix work of a step costs 3H^2*16 MAC
// at 2048 MAC/clk/CU = 0.64 us (H = 256), independent of how many of the 16 slots are used.

template <int H> struct MfGeom {
    static constexpr int NW = 8, UW = H / NW, TPW = UW / 16, KSN = H / 32;
    static constexpr int NF_G = 2 * TPW * KSN, NF_C = TPW * KSN, NF = NF_G + NF_C;   // fragments per wave
    static constexpr int PITCH = H + 8;                       // bf16 elements per LDS row of h
    static constexpr bool CAND_LDS = (H >= 256);
};

// packed[dir][wave][frag][lane][8]: frag f < NF_G: gate g = f / (TPW*KSN) (0 = r, 1 = u), else candidate
template <int H>
__global__ void __launch_bounds__(256)
gru_mfma_pack_kernel(const __bf16* W0, const __bf16* W1, __bf16* packed) {
    typedef MfGeom<H> G;
    const int total = 2 * G::NW * G::NF * 64 * 8;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        int r = idx;
        const int j = r & 7; r >>= 3;
        const int lane = r & 63; r >>= 6;
        const int f = r % G::NF; r /= G::NF;
        const int wave = r % G::NW;
        const int dir = r / G::NW;
        int g, rem;
        if (f < G::NF_G) { g = f / (G::TPW * G::KSN); rem = f % (G::TPW * G::KSN); }
        else { g = 2; rem = f - G::NF_G; }
        const int tl = rem / G::KSN, ks = rem % G::KSN;
        const int k = ks * 32 + 8 * (lane >> 4) + j;
        const int col = g * H + wave * G::UW + tl * 16 + (lane & 15);
        const __bf16* W = dir ? W1 : W0;
        packed[idx] = W[(size_t)k * 3 * H + col];
    }
}

// The two barriers of a step order LDS traffic only (h and r*h change hands through LDS): every wave's LDS operations have
// completed (lgkmcnt), nothing else is waited for -- __syncthreads() also drains vmcnt (the prefetch of the next step's
// input projections, the output stores issued just in front of barrier B).  Measured: no difference (barrier A 663, barrier
// B 576 cycles per step either way, gpurun_out r03y): the "barrier" time of this kernel is the partner wave's matrix
// products on the shared SIMD, not a memory drain.
#define GRU_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

template <int H>
__global__ void __launch_bounds__(512, 2)
gru_mfma_kernel(GruArgs a, const __bf16* packed) {
    typedef MfGeom<H> G;
    constexpr int TPW = G::TPW, KSN = G::KSN, PITCH = G::PITCH, UW = G::UW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* hb = reinterpret_cast<__bf16*>(smem);                 // [16][PITCH]
    __bf16* rhb = hb + 16 * PITCH;                                // [16][PITCH]
    bf16x8* candL = reinterpret_cast<bf16x8*>(rhb + 16 * PITCH);   // [NW][NF_C][64] when CAND_LDS

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dir = blockIdx.y, seq0 = blockIdx.x * 16;
    const int n = lane & 15, q = lane >> 4;
    const int seq = min(seq0 + n, a.n_seq - 1);
    const bool seq_ok = (seq0 + n) < a.n_seq;
    const bf16x8* pk = reinterpret_cast<const bf16x8*>(packed) + ((size_t)(dir * G::NW + wave) * G::NF) * 64 + lane;

    bf16x8 wg[G::NF_G];
#pragma unroll
    for (int f = 0; f < G::NF_G; ++f) wg[f] = pk[(size_t)f * 64];
    bf16x8 wc[G::CAND_LDS ? 1 : G::NF_C];
    if (G::CAND_LDS) {
#pragma unroll
        for (int f = 0; f < G::NF_C; ++f) candL[(wave * G::NF_C + f) * 64 + lane] = pk[(size_t)(G::NF_G + f) * 64];
    } else {
#pragma unroll
        for (int f = 0; f < G::NF_C; ++f) wc[f] = pk[(size_t)(G::NF_G + f) * 64];
    }
    for (int i = tid; i < 2 * 16 * PITCH; i += 512) hb[i] = (__bf16)0.0f;       // hb and rhb are adjacent
    float hreg[TPW][4];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl)
#pragma unroll
        for (int e = 0; e < 4; ++e) hreg[tl][e] = 0.0f;

    const int H3 = 3 * H;
    const size_t xrow = 6 * (size_t)H;
    const int ucol = wave * UW + q * 4;                          // first of this lane's 4 units in tile 0
    const float* xbase = a.xproj + (size_t)seq * a.T * xrow + (size_t)dir * H3 + ucol;
    int t = dir ? a.T - 1 : 0;
    const int dt = dir ? -1 : 1;
    f32x4 xr[TPW], xu[TPW], xc[TPW];
#pragma unroll
    for (int tl = 0; tl < TPW; ++tl) {
        const float* xp = xbase + (size_t)t * xrow + tl * 16;
        xr[tl] = *reinterpret_cast<const f32x4*>(xp);
        xu[tl] = *reinterpret_cast<const f32x4*>(xp + H);
        xc[tl] = *reinterpret_cast<const f32x4*>(xp + 2 * H);
    }
    __syncthreads();

    const __bf16* hrow = hb + n * PITCH + 8 * q;                 // B-fragment source of this lane
    const __bf16* rrow = rhb + n * PITCH + 8 * q;
    for (int step = 0; step < a.T; ++step, t += dt) {
        const bool more = step + 1 < a.T;
        const float* xn = xbase + (size_t)(more ? t + dt : t) * xrow;
        // ---- phase 1: r and u pre-activations.  All h fragments are fetched up front so the MFMA
        // chain never waits on an LDS read it has just issued.
        bf16x8 bfr[KSN];
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) bfr[ks] = *reinterpret_cast<const bf16x8*>(hrow + ks * 32);
        f32x4 ar[TPW], au[TPW];
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl) {
            ar[tl] = xr[tl];
            au[tl] = xu[tl];
            xr[tl] = *reinterpret_cast<const f32x4*>(xn + tl * 16);          // next step's, in place
            xu[tl] = *reinterpret_cast<const f32x4*>(xn + tl * 16 + H);
        }
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
#pragma unroll
            for (int tl = 0; tl < TPW; ++tl) {
                ar[tl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wg[(0 * TPW + tl) * KSN + ks], bfr[ks], ar[tl], 0, 0, 0);
                au[tl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wg[(1 * TPW + tl) * KSN + ks], bfr[ks], au[tl], 0, 0, 0);
            }
        }
        float uu[TPW][4];
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float r = fast_sigmoid(ar[tl][e]);
                uu[tl][e] = fast_sigmoid(au[tl][e]);
                o[e] = (__bf16)(r * hreg[tl][e]);
            }
            *reinterpret_cast<bf16x4*>(rhb + n * PITCH + ucol + tl * 16) = o;
        }
        GRU_LDS_BARRIER();
        // ---- phase 2: candidate, state update
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) bfr[ks] = *reinterpret_cast<const bf16x8*>(rrow + ks * 32);
        f32x4 ac[TPW];
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl) {
            ac[tl] = xc[tl];
            xc[tl] = *reinterpret_cast<const f32x4*>(xn + tl * 16 + 2 * H);
        }
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
#pragma unroll
            for (int tl = 0; tl < TPW; ++tl) {
                const bf16x8 w = G::CAND_LDS ? candL[(wave * G::NF_C + tl * KSN + ks) * 64 + lane] : wc[G::CAND_LDS ? 0 : tl * KSN + ks];
                ac[tl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, bfr[ks], ac[tl], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tl = 0; tl < TPW; ++tl) {
            bf16x4 o;
            f32x4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c = fast_tanh(ac[tl][e]);
                const float hn = uu[tl][e] * hreg[tl][e] + (1.0f - uu[tl][e]) * c;
                hreg[tl][e] = hn;
                hv[e] = hn;
                o[e] = (__bf16)hn;
            }
            *reinterpret_cast<bf16x4*>(hb + n * PITCH + ucol + tl * 16) = o;
            if (seq_ok) {
                const size_t oi = ((size_t)seq * a.T + t) * 2 * H + (size_t)dir * H + ucol + tl * 16;
                if (a.out_bf16) *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.out) + oi) = o;
                else *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + oi) = hv;
            }
        }
        GRU_LDS_BARRIER();
    }
}

template <int H>
void pack_mfma(const void* Wfw, const void* Wbw, void* packed, hipStream_t st) {
    hipLaunchKernelGGL((gru_mfma_pack_kernel<H>), dim3(256), dim3(256), 0, st, static_cast<const __bf16*>(Wfw),
                       static_cast<const __bf16*>(Wbw), static_cast<__bf16*>(packed));
}

template <int H>
int run_mfma(const GruArgs& a, const void* packed, hipStream_t st) {
    typedef MfGeom<H> G;
    const size_t lds = 2 * 16 * (size_t)G::PITCH * 2 + (G::CAND_LDS ? (size_t)G::NW * G::NF_C * 64 * 16 : 0);
    if (int rc = vc::allow_dynamic_lds<gru_mfma_kernel<H>>((int)lds)) return rc;
    hipLaunchKernelGGL((gru_mfma_kernel<H>), dim3((a.n_seq + 15) / 16, 2), dim3(512), lds, st, a,
                       static_cast<const __bf16*>(packed));
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

template <int H>
int launch_mfma(const GruArgs& a, void* ws, size_t ws_bytes, hipStream_t st) {
    const size_t need = 2 * (size_t)3 * H * H * sizeof(__bf16);
    if (ws == nullptr || ws_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_gru_bidir: workspace too small (%zu < %zu)", ws_bytes, need);
    pack_mfma<H>(a.Wh[0], a.Wh[1], ws, st);
    return run_mfma<H>(a, ws, st);
}

// ------------------------------------------------------------------------------------------
// Single-wave recurrence for small H (the encoder: H = 40): one 64-lane wave per (window,
// direction), no LDS and no barriers.  Lane j owns hidden unit j: its three weight columns
// (r_j, u_j, c_j: 3H f32 registers) and h_j.  h is broadcast to the wave one element at a time
// with v_readlane (the value becomes a scalar operand of the FMAs).
// WPB waves (= sequences) per workgroup, one per SIMD of a CU: as single-wave workgroups the 2 * n_seq
// waves were dealt to as many CUs, and a CU that holds one of them for 400 steps cannot take a
// workgroup of the register-filling MFMA kernels of the other streams (half the chip at 64 windows).
constexpr int GRU_WAVE_WPB = 4;
template <int H, typename WT>
__global__ void __launch_bounds__(64 * GRU_WAVE_WPB)
gru_wave_kernel(GruArgs a) {
    static_assert(H <= 64 && H % 4 == 0, "one lane per hidden unit, unrolled by 4");
    constexpr int H3 = 3 * H;
    const int lane = threadIdx.x & 63;
    const int seq = blockIdx.x * GRU_WAVE_WPB + (threadIdx.x >> 6), dir = blockIdx.y;
    if (seq >= a.n_seq) return;
    const bool act = lane < H;
    const int j = act ? lane : 0;
    const WT* W = reinterpret_cast<const WT*>(a.Wh[dir]);
    float wr[H], wu[H], wc[H];
#pragma unroll
    for (int k = 0; k < H; ++k) {
        wr[k] = act ? ld_w(W + (size_t)k * H3 + j) : 0.0f;
        wu[k] = act ? ld_w(W + (size_t)k * H3 + H + j) : 0.0f;
        wc[k] = act ? ld_w(W + (size_t)k * H3 + 2 * H + j) : 0.0f;
    }
    const size_t xrow = 6 * (size_t)H;
    const float* xbase = a.xproj + (size_t)seq * a.T * xrow + (size_t)dir * H3 + j;
    int t = dir ? a.T - 1 : 0;
    const int dt = dir ? -1 : 1;
    float xr = xbase[(size_t)t * xrow], xu = xbase[(size_t)t * xrow + H], xc = xbase[(size_t)t * xrow + 2 * H];
    float h = 0.0f;
    for (int step = 0; step < a.T; ++step, t += dt) {
        float xr_n = 0.0f, xu_n = 0.0f, xc_n = 0.0f;
        if (step + 1 < a.T) {
            const float* xn = xbase + (size_t)(t + dt) * xrow;
            xr_n = xn[0]; xu_n = xn[H]; xc_n = xn[2 * H];
        }
        // two partial sums per gate (four for the candidate): the FMA chains, not the issue rate,
        // bound a single wave
        float ar0 = xr, ar1 = 0.0f, au0 = xu, au1 = 0.0f;
#pragma unroll
        for (int k = 0; k < H; k += 2) {
            const float h0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h), k));
            const float h1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h), k + 1));
            ar0 = fmaf(h0, wr[k], ar0);
            au0 = fmaf(h0, wu[k], au0);
            ar1 = fmaf(h1, wr[k + 1], ar1);
            au1 = fmaf(h1, wu[k + 1], au1);
        }
        constexpr bool FAST = sizeof(WT) == 2;            // bf16 model: v_exp/v_rcp gate functions
        const float r = FAST ? fast_sigmoid(ar0 + ar1) : vc::sigmoidf_(ar0 + ar1);
        const float u = FAST ? fast_sigmoid(au0 + au1) : vc::sigmoidf_(au0 + au1);
        const float rh = r * h;
        float ac0 = xc, ac1 = 0.0f, ac2 = 0.0f, ac3 = 0.0f;
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rh), k));
            const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rh), k + 1));
            const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rh), k + 2));
            const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rh), k + 3));
            ac0 = fmaf(r0, wc[k], ac0);
            ac1 = fmaf(r1, wc[k + 1], ac1);
            ac2 = fmaf(r2, wc[k + 2], ac2);
            ac3 = fmaf(r3, wc[k + 3], ac3);
        }
        const float acs = (ac0 + ac1) + (ac2 + ac3);
        const float c = FAST ? fast_tanh(acs) : tanhf(acs);
        h = act ? (u * h + (1.0f - u) * c) : 0.0f;
        if (act) st_out<WT>(a.out, ((size_t)seq * a.T + t) * 2 * H + (size_t)dir * H + j, h, a.out_bf16);
        xr = xr_n; xu = xu_n; xc = xc_n;
    }
}

// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
softmax_argmax_kernel(const float* logits, int M, int N, int ldl, void* prob, int ldp, int out_bf16, int32_t* cls,
                      __bf16* prob2, int ldp2) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = logits + (size_t)row * ldl;
    float mx = -3.402823466e38f;
    int mi = 0x7fffffff;
    for (int c = lane; c < N; c += 64) {
        const float v = x[c];
        if (v > mx) { mx = v; mi = c; }                 // first maximum within the lane's stride
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
    }
    float s = 0.0f;
    for (int c = lane; c < N; c += 64) s += expf(x[c] - mx);
    s = vc::wave_sum(s);
    const float inv = 1.0f / s;
    const int wmax = ldp > ldp2 ? ldp : ldp2;
    for (int c = lane; c < wmax; c += 64) {
        const float p = c < N ? expf(x[c] - mx) * inv : 0.0f;
        if (c < ldp) {
            if (out_bf16) reinterpret_cast<__bf16*>(prob)[(size_t)row * ldp + c] = (__bf16)p;
            else reinterpret_cast<float*>(prob)[(size_t)row * ldp + c] = p;
        }
        if (prob2 && c < ldp2) prob2[(size_t)row * ldp2 + c] = (__bf16)p;      // second, zero-padded bf16 copy
    }
    if (cls && lane == 0) cls[row] = mi < N ? mi : 0;       // no logit above -FLT_MAX (all -inf / lowest / NaN): class 0
}

__global__ void __launch_bounds__(256)
convert_kernel(const void* src, int sdt, void* dst, int ddt, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        const float v = sdt == VC_F32 ? reinterpret_cast<const float*>(src)[i]
                                      : (float)reinterpret_cast<const __bf16*>(src)[i];
        if (ddt == VC_F32) reinterpret_cast<float*>(dst)[i] = v;
        else reinterpret_cast<__bf16*>(dst)[i] = (__bf16)v;
    }
}

// ------------------------------------------------------------------------------------------
// Which of the two bf16 forms (H = 128 / 256) a packed-weights call takes.  Measured alone on an MI355X (256 CUs) at 64
// windows x 400 steps, weights packed beforehand (profiles/gru_modes/README.md):
//   resident (one sequence per workgroup, weights in VGPRs, 2 * n_seq workgroups): H = 256 1.45 us/step, H = 128 0.92;
//   MFMA (16 sequences per workgroup, 2 * ceil(n_seq / 16) workgroups):             H = 256 1.86 us/step, H = 128 0.92.
// A resident workgroup of H = 256 fills its CU's register file, so the form keeps its per-step figure only while every
// workgroup has a CU to itself: the makespan of one call is smallest with the resident form when its 2 * n_seq
// workgroups fit ONE round of the device's CUs, and with the MFMA form beyond (a second round doubles the resident
// time).  That is the rule at H = 256.  At H = 128 the two forms tie at 64 windows (the step is barrier-bound either
// way), so that size keeps the rule it had: resident below 32 sequences, MFMA -- sixteen times fewer CUs for the same
// time -- from 32 up.  These are the library's defaults, which serve a caller with one batch in flight.  A caller that
// keeps several batches in flight wants the CUs for the MFMA-bound launches of its other streams and forces the MFMA
// form (gru_mfma = 1, part of _vc.throughput_mode(): +7.7 % frames/s at 64 windows with ten steps in flight);
// gru_mfma = 0 forces the resident form.
int gru_pick_form(int H, int w_dtype, int n_seq, int n_cu, int gm) {
    if (w_dtype != VC_BF16 || (H != 128 && H != 256) || n_seq <= 0) return VC_GRU_FORM_NONE;
    if (gm >= 0) return gm == 1 ? VC_GRU_FORM_MFMA : VC_GRU_FORM_RESIDENT;
    if (H == 128) return n_seq < 32 ? VC_GRU_FORM_RESIDENT : VC_GRU_FORM_MFMA;
    return 2 * (long long)n_seq <= n_cu ? VC_GRU_FORM_RESIDENT : VC_GRU_FORM_MFMA;
}

// CU count of the current device, asked once per device.
int device_cu_count(int* n_cu) {
    constexpr int MAX_DEV = 64;
    static std::atomic<int> cached[MAX_DEV];
    int dev = 0;
    VC_HIP_CHECK(hipGetDevice(&dev));
    if (dev >= 0 && dev < MAX_DEV) {
        const int c = cached[dev].load(std::memory_order_relaxed);
        if (c > 0) { *n_cu = c; return VC_OK; }
    }
    int c = 0;
    VC_HIP_CHECK(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev));
    if (dev >= 0 && dev < MAX_DEV) cached[dev].store(c, std::memory_order_relaxed);
    *n_cu = c;
    return VC_OK;
}

bool gru_form_ok(int form, int H, int w_dtype) {
    return (form == VC_GRU_FORM_RESIDENT || form == VC_GRU_FORM_MFMA) && w_dtype == VC_BF16 && (H == 128 || H == 256);
}

}  // namespace

extern "C" {

size_t vc_gru_workspace_bytes(int32_t H, int32_t w_dtype) {
    if (H <= 0) return 0;
    return 2 * (size_t)3 * H * H * (w_dtype == VC_F32 ? 4 : 2);
}

int vc_gru_bidir(const float* d_xproj, const void* d_Wh_fw, const void* d_Wh_bw, int32_t w_dtype, int32_t n_seq,
                 int32_t T, int32_t H, void* d_out, int32_t out_dtype, void* d_workspace, size_t workspace_bytes,
                 void* stream) {
    VC_REQUIRE(d_xproj && d_Wh_fw && d_Wh_bw && d_out, "NULL argument");
    VC_REQUIRE(n_seq > 0 && T > 0 && H > 0 && H <= GEN_H_MAX, "bad shape n_seq=%d T=%d H=%d", n_seq, T, H);
    VC_REQUIRE(w_dtype == VC_F32 || w_dtype == VC_BF16, "bad w_dtype %d", w_dtype);
    VC_REQUIRE(out_dtype == VC_F32 || out_dtype == VC_BF16, "bad out_dtype %d", out_dtype);
    GruArgs a;
    a.xproj = d_xproj; a.Wh[0] = d_Wh_fw; a.Wh[1] = d_Wh_bw; a.out = d_out;
    a.n_seq = n_seq; a.T = T; a.H = H; a.out_bf16 = out_dtype == VC_BF16;
    const size_t wbytes = (size_t)H * 3 * H * (w_dtype == VC_F32 ? 4 : 2);
    const size_t base = 3 * (size_t)H * 4;
    a.w_in_lds = (base + wbytes <= 150 * 1024);
    const size_t lds = base + (a.w_in_lds ? wbytes : 0);
    int nt = 256;
    while (nt < GEN_NT_MAX && nt < 2 * H) nt *= 2;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(n_seq, 2);
    // The decoder's sizes in bf16 have two forms (figures and the reasoning: gru_pick_form above).  This entry point packs
    // the weights into the workspace on every call and keeps the rule its callers know: the resident form below 32
    // sequences, the MFMA form from 32 up; vc_set_option("gru_mfma", 0 / 1) forces either.  The packed-weights entry
    // point (vc_gru_bidir_packed with the form vc_gru_form names) chooses by makespan from the device's CU count.
    const int gm = vc::opt(vc::OPT_GRU_MFMA);
    const bool use_valu = gm >= 0 ? (gm != 1) : (n_seq < 32);
    if (w_dtype == VC_BF16 && H == 256) return use_valu ? launch_resident<256, __bf16, 512>(a, d_workspace, workspace_bytes, st)
                                                        : launch_mfma<256>(a, d_workspace, workspace_bytes, st);
    if (w_dtype == VC_BF16 && H == 128) return use_valu ? launch_resident<128, __bf16, 256>(a, d_workspace, workspace_bytes, st)
                                                        : launch_mfma<128>(a, d_workspace, workspace_bytes, st);
    // (H = 128 runs 256 threads: four fat waves beat sixteen thin ones, the step is barrier-bound)
    if (w_dtype == VC_F32 && H == 128) return launch_resident<128, float, 1024>(a, d_workspace, workspace_bytes, st);
    if (H == 40) {                                      // the shipped encoder (hp/encoder_cfg_d.json)
        const dim3 gw((n_seq + GRU_WAVE_WPB - 1) / GRU_WAVE_WPB, 2);
        if (w_dtype == VC_F32) hipLaunchKernelGGL((gru_wave_kernel<40, float>), gw, dim3(64 * GRU_WAVE_WPB), 0, st, a);
        else hipLaunchKernelGGL((gru_wave_kernel<40, __bf16>), gw, dim3(64 * GRU_WAVE_WPB), 0, st, a);
        VC_HIP_CHECK(hipGetLastError());
        return VC_OK;
    }
    if (w_dtype == VC_F32) {
        VC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gru_generic_kernel<float>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(gru_generic_kernel<float>, grid, dim3(nt), lds, st, a);
    } else {
        VC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gru_generic_kernel<__bf16>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(gru_generic_kernel<__bf16>, grid, dim3(nt), lds, st, a);
    }
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int32_t vc_gru_form(int32_t H, int32_t w_dtype, int32_t n_seq, int32_t n_cu) {
    const int gm = vc::opt(vc::OPT_GRU_MFMA);
    if (n_cu <= 0 && gm < 0 && H == 256 && w_dtype == VC_BF16 && device_cu_count(&n_cu) != VC_OK) return -1;
    return gru_pick_form(H, w_dtype, n_seq, n_cu, gm);
}

size_t vc_gru_packed_bytes(int32_t form, int32_t H, int32_t w_dtype) {
    return gru_form_ok(form, H, w_dtype) ? 2 * (size_t)3 * H * H * 2 : 0;
}

int vc_gru_pack(int32_t form, const void* d_Wh_fw, const void* d_Wh_bw, int32_t w_dtype, int32_t H, void* d_packed,
                size_t packed_bytes, void* stream) {
    VC_REQUIRE(d_Wh_fw && d_Wh_bw && d_packed, "vc_gru_pack: NULL argument");
    VC_REQUIRE(reinterpret_cast<uintptr_t>(d_packed) % 16 == 0, "vc_gru_pack: d_packed is not 16-byte aligned");
    VC_REQUIRE(gru_form_ok(form, H, w_dtype), "vc_gru_pack: no packed form %d for H=%d w_dtype=%d", form, H, w_dtype);
    const size_t need = vc_gru_packed_bytes(form, H, w_dtype);
    if (packed_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_gru_pack: image buffer too small (%zu < %zu)", packed_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (form == VC_GRU_FORM_RESIDENT) {
        if (H == 256) pack_resident<256, __bf16, 512>(d_Wh_fw, d_Wh_bw, d_packed, st);
        else pack_resident<128, __bf16, 256>(d_Wh_fw, d_Wh_bw, d_packed, st);
    } else {
        if (H == 256) pack_mfma<256>(d_Wh_fw, d_Wh_bw, d_packed, st);
        else pack_mfma<128>(d_Wh_fw, d_Wh_bw, d_packed, st);
    }
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_gru_bidir_packed(int32_t form, const float* d_xproj, const void* d_packed, size_t packed_bytes, int32_t w_dtype,
                        int32_t n_seq, int32_t T, int32_t H, void* d_out, int32_t out_dtype, void* stream) {
    VC_REQUIRE(d_xproj && d_packed && d_out, "vc_gru_bidir_packed: NULL argument");
    VC_REQUIRE(reinterpret_cast<uintptr_t>(d_packed) % 16 == 0, "vc_gru_bidir_packed: d_packed is not 16-byte aligned");
    VC_REQUIRE(n_seq > 0 && T > 0, "vc_gru_bidir_packed: bad shape n_seq=%d T=%d", n_seq, T);
    VC_REQUIRE(gru_form_ok(form, H, w_dtype), "vc_gru_bidir_packed: no packed form %d for H=%d w_dtype=%d", form, H, w_dtype);
    VC_REQUIRE(out_dtype == VC_F32 || out_dtype == VC_BF16, "bad out_dtype %d", out_dtype);
    const size_t need = vc_gru_packed_bytes(form, H, w_dtype);
    if (packed_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_gru_bidir_packed: image too small (%zu < %zu)", packed_bytes, need);
    GruArgs a;
    a.xproj = d_xproj; a.Wh[0] = a.Wh[1] = nullptr; a.out = d_out;             // the packed kernels never read Wh
    a.n_seq = n_seq; a.T = T; a.H = H; a.out_bf16 = out_dtype == VC_BF16; a.w_in_lds = 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (form == VC_GRU_FORM_RESIDENT)
        return H == 256 ? run_resident<256, __bf16, 512>(a, d_packed, st) : run_resident<128, __bf16, 256>(a, d_packed, st);
    return H == 256 ? run_mfma<256>(a, d_packed, st) : run_mfma<128>(a, d_packed, st);
}

int vc_lstm_bidir(const float* d_xproj, const void* d_Wh_fw, const void* d_Wh_bw, int32_t w_dtype, int32_t n_seq, int32_t T,
                  int32_t H, void* d_out, int32_t out_dtype, void* stream) {
    VC_REQUIRE(d_xproj && d_Wh_fw && d_Wh_bw && d_out, "NULL argument");
    VC_REQUIRE(n_seq > 0 && T > 0 && H > 0 && H <= 512 && n_seq <= 65535, "vc_lstm_bidir: bad shape n_seq=%d T=%d H=%d (H <= 512)", n_seq, T, H);
    VC_REQUIRE((w_dtype == VC_F32 || w_dtype == VC_BF16) && (out_dtype == VC_F32 || out_dtype == VC_BF16), "bad dtype");
    LstmArgs a;
    a.xproj = d_xproj; a.Wh[0] = d_Wh_fw; a.Wh[1] = d_Wh_bw; a.n_seq = n_seq; a.T = T; a.H = H;
    a.out = d_out; a.out_bf16 = out_dtype == VC_BF16;
    const size_t base = (size_t)5 * H * sizeof(float);
    const size_t wbytes = (size_t)4 * H * H * (w_dtype == VC_F32 ? 4 : 2);
    a.w_in_lds = (base + wbytes <= 150 * 1024);
    const size_t lds = base + (a.w_in_lds ? wbytes : 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (w_dtype == VC_F32) {
        VC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_generic_kernel<float>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(lstm_generic_kernel<float>, dim3(n_seq, 2), dim3(512), lds, st, a);
    } else {
        VC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lstm_generic_kernel<__bf16>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(lstm_generic_kernel<__bf16>, dim3(n_seq, 2), dim3(512), lds, st, a);
    }
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_softmax_argmax(const float* d_logits, int32_t M, int32_t N, int32_t ldl, void* d_prob, int32_t ldp,
                      int32_t out_dtype, int32_t* d_class, void* stream) {
    VC_REQUIRE(d_logits && d_prob, "NULL argument");
    VC_REQUIRE(M > 0 && N > 0 && ldl >= N && ldp >= N, "bad shape M=%d N=%d ldl=%d ldp=%d", M, N, ldl, ldp);
    VC_REQUIRE(out_dtype == VC_F32 || out_dtype == VC_BF16, "bad out_dtype %d", out_dtype);
    hipLaunchKernelGGL(softmax_argmax_kernel, dim3((M + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_logits, M, N, ldl, d_prob, ldp, out_dtype == VC_BF16, d_class, static_cast<__bf16*>(nullptr), 0);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_softmax_argmax_dual(const float* d_logits, int32_t M, int32_t N, int32_t ldl, float* d_prob, int32_t ldp,
                           void* d_prob_bf16, int32_t ldp_bf16, int32_t* d_class, void* stream) {
    VC_REQUIRE(d_logits && d_prob && d_prob_bf16, "NULL argument");
    VC_REQUIRE(M > 0 && N > 0 && ldl >= N && ldp >= N && ldp_bf16 >= N, "bad shape M=%d N=%d ldl=%d ldp=%d/%d", M, N, ldl, ldp, ldp_bf16);
    hipLaunchKernelGGL(softmax_argmax_kernel, dim3((M + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_logits, M, N, ldl, static_cast<void*>(d_prob), ldp, 0, d_class, static_cast<__bf16*>(d_prob_bf16), ldp_bf16);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_convert(const void* d_src, int32_t src_dtype, void* d_dst, int32_t dst_dtype, size_t n, void* stream) {
    VC_REQUIRE(d_src && d_dst, "NULL argument");
    VC_REQUIRE((src_dtype == VC_F32 || src_dtype == VC_BF16) && (dst_dtype == VC_F32 || dst_dtype == VC_BF16), "bad dtype");
    if (n == 0) return VC_OK;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(convert_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_src, src_dtype,
                       d_dst, dst_dtype, n);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
