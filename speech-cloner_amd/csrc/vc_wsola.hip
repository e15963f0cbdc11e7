// Time scaling of a waveform on the device (include/vc_hip.h, "Time scale"): waveform-similarity overlap-add along the
// integer time map that vc_duration_map writes.
//
//   wsola_plan_kernel  x [B, x_stride], len, pos [B, out_frames] (Q16 frames), n_out -> per grain its input position a_k and
//                      the cost it was chosen at; the grain count K and the output length.  Integers only.
//   wsola_ola_kernel   x, the plan, the cross-fade table T [S] -> y [B, hop * (out_frames - 1)]: every output sample is a
//                      cross-fade of two input samples.  A gather: no atomics, every output element written once.
//
// wsola_plan_kernel: one workgroup of 512 lanes per utterance, because a_k depends on a_{k-1}.  Per step the 2 S reference
// samples (from a_{k-1} on) and the 2 S + 2 tol samples every candidate window lies in go from global memory into LDS,
// quantised on the way to 16 bits with a bias of 32,768 and packed two to a dword (4 KB + 8 KB at the limits).  Candidates
// go in PAIRS (2 p and 2 p + 1, d = c - tol): both windows lie in the same dwords, the odd one a sample on, so one LDS read
// per dword serves both -- the odd window's dword is put together from two neighbours with one v_alignbit -- against four
// reference dwords from one 16-byte read of the same address in every lane (a broadcast); one v_sad_u16 adds both absolute
// differences of a dword.  Neighbouring lanes read neighbouring dwords.  With 256 pairs or fewer, G = min(512 / pairs, 8)
// lanes share a window, a segment each, and the partial sums meet in LDS (a third barrier); with more, lane t takes whole
// windows t, t + 512, ...
// The key (cost, |d|, d) is 64 bits wide: minimum over the wave in two DPP reductions (the cost, then the rest among the
// lanes that hold it), over the eight waves through LDS.  Reference and span are staged in ONE loop of unconditional loads
// (indices clamped into the signal, the value chosen afterwards), so a step waits for one round trip to L2, not four.  The
// targets tau_k do not depend on the chain: they are computed 512 steps at a time, one per lane, into LDS, and the results
// leave 512 steps at a time too, so no store's acknowledgement is waited for inside a step.  The candidate span of the next
// step is NOT staged ahead.
// Loop bounds come from out_frames, hop, S and tol; len and n_out are clamped, every pos is clamped when read, and a sample
// index outside [0, len) is never an address (it reads as 0).
//
// wsola_ola_kernel: grid (tiles of 1,024 outputs, B), 256 lanes, lane t owns samples t, t + 256, ... of the tile, so adjacent
// lanes read adjacent input samples of the same grain.
#include <cmath>
#include <climits>
#include "vc_common.h"

namespace {

constexpr int NT_W = 512;               // lanes of the plan kernel
constexpr int NW_W = NT_W / 64;
constexpr int MAX_G = 8;                // lanes that share one window at most
constexpr int OT_W = 256;               // lanes of the overlap-add kernel
constexpr int OV_W = 4;                 // samples per lane
constexpr int TILE_W = OT_W * OV_W;
constexpr int MAX_LEN_W = 1 << 24, MAX_OUT_FRAMES = 16384, MAX_HOP_W = 1024, MAX_S = 1024, MAX_TOL = 1024;
constexpr int A_GUARD = 1 << 24;
constexpr int REF_DW = MAX_S;                                       // 2 S samples, two to a dword
constexpr int CAND_DW = MAX_S + MAX_TOL + 1;                        // 2 S + 2 tol samples and one dword for the odd windows

// clamp(rint(x * qscale), -32767, 32767) + 32768 in [1, 65535]; NaN gives 32768 (q = 0)
__device__ __forceinline__ unsigned quantise_biased(float x, float qscale) {
    const float p = x * qscale;
    float r = rintf(p);
    r = fminf(fmaxf(r, -32767.0f), 32767.0f);
    if (p != p) r = 0.0f;
    return (unsigned)((int)r + 32768);
}

// the dword that holds samples i and i + 1 of x~ (zero outside [0, len), len >= 1).  Both loads are unconditional, from
// indices clamped into the signal, so they leave together and nothing at or beyond len is read; the value is chosen after.
__device__ __forceinline__ unsigned stage_pair(const float* __restrict__ x, int i, int len, float qscale) {
    const float v0 = x[min(max(i, 0), len - 1)];
    const float v1 = x[min(max(i + 1, 0), len - 1)];
    const unsigned lo = (i >= 0 && i < len) ? quantise_biased(v0, qscale) : 32768u;
    const unsigned hi = (i + 1 >= 0 && i + 1 < len) ? quantise_biased(v1, qscale) : 32768u;
    return lo | (hi << 16);
}

__device__ __forceinline__ int target_of(int pos_q, int hop, int len) {
    const long long p = pos_q > 0 ? pos_q : 0;
    const long long tau = (p * hop + 32768) >> 16;
    return (int)min(max(tau, 0LL), (long long)(len - 1));
}

// The least value over the wave, in every lane: the DPP steps of vc_common.h's float reductions (quad swaps, half-row and
// row mirrors, the row_bcast:15 / row_bcast:31 carries, one v_readlane) on unsigned integers.  A lane whose source a step
// disables takes the seed, the greatest value.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_min_u32(unsigned v) {
    return min(v, (unsigned)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = dpp_min_u32<0xB1, 0xF>(v);      // quad_perm [1,0,3,2]
    v = dpp_min_u32<0x4E, 0xF>(v);      // quad_perm [2,3,0,1]
    v = dpp_min_u32<0x141, 0xF>(v);     // row_half_mirror
    v = dpp_min_u32<0x140, 0xF>(v);     // row_mirror: every lane of a row of 16
    v = dpp_min_u32<0x142, 0xA>(v);     // row_bcast:15 into rows 1 and 3
    v = dpp_min_u32<0x143, 0xC>(v);     // row_bcast:31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Dwords [j0, j1) of the two windows that start at dword w[0] -- on its even and on its odd sample -- against the reference:
// acc0 and acc1 take their sums of absolute differences.  j0 is a multiple of 4 (the reference is read 16 bytes at a time,
// the same address in every lane); eight dwords an iteration where they last, so that ten LDS reads are in flight at once.
__device__ __forceinline__ void sad4(unsigned& lo, unsigned h0, unsigned h1, unsigned h2, unsigned h3, uint4 r, unsigned& acc0, unsigned& acc1) {
    acc0 = __builtin_amdgcn_sad_u16(lo, r.x, acc0);
    acc1 = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbit(h0, lo, 16), r.x, acc1);
    acc0 = __builtin_amdgcn_sad_u16(h0, r.y, acc0);
    acc1 = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbit(h1, h0, 16), r.y, acc1);
    acc0 = __builtin_amdgcn_sad_u16(h1, r.z, acc0);
    acc1 = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbit(h2, h1, 16), r.z, acc1);
    acc0 = __builtin_amdgcn_sad_u16(h2, r.w, acc0);
    acc1 = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbit(h3, h2, 16), r.w, acc1);
    lo = h3;
}
__device__ __forceinline__ void window_sad(const unsigned* w, const uint4* ref4, int j0, int j1, unsigned& acc0, unsigned& acc1) {
    const unsigned* ref = reinterpret_cast<const unsigned*>(ref4);
    unsigned lo = w[j0];
    int j = j0;
    for (; j + 8 <= j1; j += 8) {
        const uint4 r0 = ref4[j >> 2], r1 = ref4[(j >> 2) + 1];
        const unsigned h0 = w[j + 1], h1 = w[j + 2], h2 = w[j + 3], h3 = w[j + 4], h4 = w[j + 5], h5 = w[j + 6], h6 = w[j + 7], h7 = w[j + 8];
        sad4(lo, h0, h1, h2, h3, r0, acc0, acc1);
        sad4(lo, h4, h5, h6, h7, r1, acc0, acc1);
    }
    for (; j + 4 <= j1; j += 4) sad4(lo, w[j + 1], w[j + 2], w[j + 3], w[j + 4], ref4[j >> 2], acc0, acc1);
    for (; j < j1; ++j) {
        const unsigned hi = w[j + 1], r = ref[j];
        acc0 = __builtin_amdgcn_sad_u16(lo, r, acc0);
        acc1 = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbit(hi, lo, 16), r, acc1);
        lo = hi;
    }
}

// (cost, |d|, d) as one ordered 64-bit key
__device__ __forceinline__ unsigned long long cost_key(unsigned cost, int d) {
    return ((unsigned long long)cost << 32) | ((unsigned)(d < 0 ? -d : d) << 16) | (unsigned)(d + MAX_TOL);
}

// the better key of pair p: candidates 2 p and 2 p + 1 (d = c - tol); the last pair holds one candidate, 2 tol
__device__ __forceinline__ unsigned long long pair_key(unsigned acc0, unsigned acc1, int p, int tol) {
    const int d = 2 * p - tol;
    const unsigned long long k0 = cost_key(acc0, d);
    return p < tol ? min(k0, cost_key(acc1, d + 1)) : k0;
}

struct WsolaPlanArgs {
    const float* x;                     // [B, x_stride]
    const int32_t* len;                 // [B]
    const int32_t* pos;                 // [B, out_frames]
    const int32_t* n_out;               // [B]
    int x_stride, max_len, out_frames, hop, group, tol, M;
    float qscale;
    int32_t* a;                         // [B, M]
    int32_t* cost;                      // [B, M]
    int32_t* n_grains;                  // [B]
    int32_t* out_len;                   // [B]
};

__global__ void __launch_bounds__(NT_W)
wsola_plan_kernel(const WsolaPlanArgs g) {
    __shared__ uint4 ref4[REF_DW / 4];                              // read four dwords at a time: the same address in every lane
    __shared__ unsigned cand[CAND_DW];
    unsigned* const ref = reinterpret_cast<unsigned*>(ref4);
    __shared__ unsigned long long wkey[NW_W];
    __shared__ unsigned part[2][NT_W];                              // partial sums of the lanes that share a window
    __shared__ int taus[NT_W], res_a[NT_W], res_c[NT_W];              // 512 steps' targets and results: no global access per step but the staging
    const int t = threadIdx.x, b = blockIdx.x;
    const int len = min(max(g.len[b], 0), g.max_len);
    const int n_out = min(max(g.n_out[b], 0), g.out_frames);
    const int S = g.group * g.hop, tol = g.tol;
    const int out_len = (n_out >= 2 && len >= 1) ? g.hop * (n_out - 1) : 0;
    const int K = out_len > 0 ? min((out_len + S - 1) / S + 1, g.M) : 0;       // (never less: M is K at n_out == out_frames)
    const float* x = g.x + (size_t)b * g.x_stride;
    const int32_t* pos = g.pos + (size_t)b * g.out_frames;
    int32_t* a_row = g.a + (size_t)b * g.M;
    int32_t* c_row = g.cost + (size_t)b * g.M;
    if (t == 0) { g.n_grains[b] = K; g.out_len[b] = out_len; }
    for (int k = K + t; k < g.M; k += NT_W) { a_row[k] = INT_MIN; c_row[k] = -1; }
    if (K == 0) return;                                             // (uniform: no lane reaches a barrier)
    int a_prev = target_of(pos[0], g.hop, len);                     // a_0 = tau_0
    if (t == 0) { a_row[0] = a_prev; c_row[0] = 0; }
    const int n_pair = tol + 1, cand_dw = S + tol + 1;
    // Up to 255 pairs, G = min(512 / pairs, 8) lanes share a window: lane t takes segment t / pairs of pair t % pairs, dwords
    // [seg_j0, seg_j1) with the inner bounds at multiples of 4.  One wave per SIMD walking a whole window waits for an LDS
    // round trip per few dwords; sharing it shortens that chain G-fold.
    const int G = n_pair >= NT_W / 2 + 1 ? 1 : min(NT_W / n_pair, MAX_G);
    const int seg = t / n_pair, pr = t - seg * n_pair;
    const int seg_j0 = (seg * S / G) & ~3, seg_j1 = seg >= G - 1 ? S : ((seg + 1) * S / G) & ~3;
    for (int k = 1; k < K; ++k) {
        const int slot = (k - 1) & (NT_W - 1);
        if (slot == 0) {                                            // the targets of the next 512 steps, one per lane (uniform branch;
            const long long kk = (long long)k + t;                  //  the last reads of the old ones lie two barriers back)
            if (kk < K) taus[t] = target_of(pos[(int)min(kk * g.group, (long long)(n_out - 1))], g.hop, len);
            __syncthreads();
            if (k > 1) { a_row[k - NT_W + t] = res_a[t]; c_row[k - NT_W + t] = res_c[t]; }          // the results of the last 512 steps
        }
        const int tau = taus[slot];
        const int base = tau - tol - S;                             // sample 0 of the candidate span
        for (int j = t; j < S + cand_dw; j += NT_W) {               // one loop: the reference's and the span's loads leave together
            const bool is_ref = j < S;
            const unsigned v = stage_pair(x, is_ref ? a_prev + 2 * j : base + 2 * (j - S), len, g.qscale);
            if (is_ref) ref[j] = v; else cand[j - S] = v;
        }
        __syncthreads();
        unsigned long long best = ~0ULL;
        if (G == 1) {                                               // (uniform) 256 pairs or more: whole windows, in rounds of 512
            for (int p = t; p < n_pair; p += NT_W) {
                unsigned acc0 = 0, acc1 = 0;
                window_sad(cand + p, ref4, 0, S, acc0, acc1);
                best = min(best, pair_key(acc0, acc1, p, tol));
            }
        } else {                                                    // fewer: G lanes share a window, the partial sums meet in LDS
            if (seg < G) {
                unsigned acc0 = 0, acc1 = 0;
                window_sad(cand + pr, ref4, seg_j0, seg_j1, acc0, acc1);
                part[0][t] = acc0; part[1][t] = acc1;
            }
            __syncthreads();
            if (t < n_pair) {
                unsigned acc0 = 0, acc1 = 0;
                for (int q = 0; q < G; ++q) { acc0 += part[0][q * n_pair + t]; acc1 += part[1][q * n_pair + t]; }
                best = pair_key(acc0, acc1, t, tol);
            }
        }
        {                                                           // the wave's least key: first the cost, then (|d|, d) among its holders
            const unsigned c_lane = (unsigned)(best >> 32);
            const unsigned c_min = wave_min_u32(c_lane);
            const unsigned d_min = wave_min_u32(c_lane == c_min ? (unsigned)best : 0xFFFFFFFFu);
            best = ((unsigned long long)c_min << 32) | d_min;
        }
        if ((t & 63) == 0) wkey[t >> 6] = best;
        __syncthreads();
        best = wkey[0];
#pragma unroll
        for (int w = 1; w < NW_W; ++w) best = wkey[w] < best ? wkey[w] : best;
        a_prev = tau + (int)(best & 0xFFFFu) - MAX_TOL;
        if (t == 0) { res_a[slot] = a_prev; res_c[slot] = (int)(best >> 32); }
    }
    __syncthreads();
    const int k0 = ((K - 2) & ~(NT_W - 1)) + 1;                     // the step of the last refill: what was chosen since goes out now
    if (k0 + t < K) { a_row[k0 + t] = res_a[t]; c_row[k0 + t] = res_c[t]; }
}

__device__ __forceinline__ float lerp_rn(float x0, float x1, float w) {
#pragma clang fp contract(off)
    const float d = x1 - x0;
    const float m = w * d;
    return x0 + m;
}

__global__ void __launch_bounds__(OT_W)
wsola_ola_kernel(const float* __restrict__ x, int x_stride, const int32_t* __restrict__ len_all, const int32_t* __restrict__ a_all,
                 const int32_t* __restrict__ n_grains_all, const int32_t* __restrict__ out_len_all, const float* __restrict__ T,
                 int max_len, int M, int S, int L, float* __restrict__ y) {
    const int t = threadIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.x * TILE_W;
    const int len = min(max(len_all[b], 0), max_len);
    const int out_len = min(max(out_len_all[b], 0), L);
    const int K = min(max(n_grains_all[b], 0), M);
    const float* xb = x + (size_t)b * x_stride;
    const int32_t* a = a_all + (size_t)b * M;
    float* yb = y + (size_t)b * L;
#pragma unroll
    for (int v = 0; v < OV_W; ++v) {
        const int m = t0 + t + v * OT_W;
        if (m >= L) break;
        float out = 0.0f;
        if (m < out_len) {
            const int k = m / S, r = m - k * S;
            float A = 0.0f, B = 0.0f;
            if (k < K) {
                const int ak = a[k];
                if (ak >= -A_GUARD && ak <= A_GUARD) {
                    const int i = ak + r;
                    if (i >= 0 && i < len) A = xb[i];
                }
            }
            if (k + 1 < K) {
                const int ak = a[k + 1];
                if (ak >= -A_GUARD && ak <= A_GUARD) {
                    const int i = ak + r - S;
                    if (i >= 0 && i < len) B = xb[i];
                }
            }
            out = lerp_rn(A, B, T[r]);
        }
        yb[m] = out;
    }
}

inline bool wsola_limits_ok(int batch, int max_len, int out_frames, int hop, int group, int tol, bool& shape_ok) {
    shape_ok = batch >= 1 && max_len >= 1 && out_frames >= 1 && hop >= 1 && group >= 1 && tol >= 0;
    if (!shape_ok) return false;
    return batch <= 65535 && max_len <= MAX_LEN_W && out_frames <= MAX_OUT_FRAMES && hop <= MAX_HOP_W && group <= MAX_S &&
           (long long)group * hop <= MAX_S && tol <= MAX_TOL;
}

int wsola_refuse(const char* who, int batch, int max_len, int out_frames, int hop, int group, int tol) {
    return vc::set_error(VC_ERR_UNSUPPORTED, "%s: limits are batch <= 65535, max_len <= %d, out_frames <= %d, hop <= %d, "
                         "group * hop <= %d and tol <= %d; got batch %d, max_len %d, out_frames %d, hop %d, group %d, tol %d", who,
                         MAX_LEN_W, MAX_OUT_FRAMES, MAX_HOP_W, MAX_S, MAX_TOL, batch, max_len, out_frames, hop, group, tol);
}

}  // namespace

extern "C" {

int32_t vc_wsola_max_grains(int32_t out_frames, int32_t hop, int32_t group) {
    bool shape_ok;
    if (!wsola_limits_ok(1, 1, out_frames, hop, group, 0, shape_ok)) return 0;
    const int S = group * hop;
    return (hop * (out_frames - 1) + S - 1) / S + 1;
}

int vc_wsola_plan(const float* d_x, int32_t x_stride, const int32_t* d_len, const int32_t* d_pos, const int32_t* d_n_out,
                  int32_t batch, int32_t max_len, int32_t out_frames, int32_t hop, int32_t group, int32_t tol, float qscale,
                  int32_t* d_a, int32_t* d_cost, int32_t* d_n_grains, int32_t* d_out_len, void* stream) {
    VC_REQUIRE(d_x && d_len && d_pos && d_n_out && d_a && d_cost && d_n_grains && d_out_len, "vc_wsola_plan: NULL argument");
    bool shape_ok;
    const bool ok = wsola_limits_ok(batch, max_len, out_frames, hop, group, tol, shape_ok);
    VC_REQUIRE(shape_ok, "vc_wsola_plan: bad shape (batch %d, max_len %d, out_frames %d, hop %d, group %d, tol %d)", batch, max_len,
               out_frames, hop, group, tol);
    VC_REQUIRE(x_stride >= max_len, "vc_wsola_plan: x_stride %d is below max_len %d", x_stride, max_len);
    VC_REQUIRE(qscale > 0.0f && qscale <= 3.0e38f, "vc_wsola_plan: qscale must be positive and finite");
    if (!ok) return wsola_refuse("vc_wsola_plan", batch, max_len, out_frames, hop, group, tol);
    WsolaPlanArgs g;
    g.x = d_x; g.len = d_len; g.pos = d_pos; g.n_out = d_n_out; g.x_stride = x_stride; g.max_len = max_len;
    g.out_frames = out_frames; g.hop = hop; g.group = group; g.tol = tol; g.M = vc_wsola_max_grains(out_frames, hop, group);
    g.qscale = qscale; g.a = d_a; g.cost = d_cost; g.n_grains = d_n_grains; g.out_len = d_out_len;
    hipLaunchKernelGGL(wsola_plan_kernel, dim3(batch), dim3(NT_W), 0, static_cast<hipStream_t>(stream), g);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_wsola_ola_f32(const float* d_x, int32_t x_stride, const int32_t* d_len, const int32_t* d_a, const int32_t* d_n_grains,
                     const int32_t* d_out_len, const float* d_window, int32_t batch, int32_t max_len, int32_t out_frames,
                     int32_t hop, int32_t group, float* d_y, void* stream) {
    VC_REQUIRE(d_x && d_len && d_a && d_n_grains && d_out_len && d_window, "vc_wsola_ola_f32: NULL argument");
    bool shape_ok;
    const bool ok = wsola_limits_ok(batch, max_len, out_frames, hop, group, 0, shape_ok);
    VC_REQUIRE(shape_ok, "vc_wsola_ola_f32: bad shape (batch %d, max_len %d, out_frames %d, hop %d, group %d)", batch, max_len,
               out_frames, hop, group);
    VC_REQUIRE(x_stride >= max_len, "vc_wsola_ola_f32: x_stride %d is below max_len %d", x_stride, max_len);
    if (!ok) return wsola_refuse("vc_wsola_ola_f32", batch, max_len, out_frames, hop, group, 0);
    const int L = hop * (out_frames - 1);
    if (L == 0) return VC_OK;                                       // a row of no samples: nothing to write
    VC_REQUIRE(d_y && d_y != d_x, "vc_wsola_ola_f32: d_y is NULL or d_x");
    hipLaunchKernelGGL(wsola_ola_kernel, dim3((L + TILE_W - 1) / TILE_W, batch), dim3(OT_W), 0, static_cast<hipStream_t>(stream),
                       d_x, x_stride, d_len, d_a, d_n_grains, d_out_len, d_window, max_len, vc_wsola_max_grains(out_frames, hop, group),
                       group * hop, L, d_y);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
