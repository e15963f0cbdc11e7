// Pitch conversion on the device (include/vc_hip.h, "Pitch"): overlap-add of grains placed by integrating an F0 track.
//
//   psola_plan_kernel  period_q, ratio_q [B, F] (Q16) + len -> the analysis marks a, the synthesis marks s, and per
//                      synthesis mark its grain: src (the nearest analysis mark) and h (the half width).  Integers only.
//   psola_ola_kernel   x [B, Lmax], the plan, the window table -> y [B, Lmax]: every output sample gathers the grains
//                      that cover it, N / max(D, w_floor).  No atomics, every output element written once.
//
// psola_plan_kernel: one workgroup of 256 lanes per utterance.  The step of the mark recurrence is constant inside a
// frame, so the recurrence runs over FRAMES, not marks: the tables go through LDS in tiles of 1,024 frames (all lanes load
// and clamp them and derive the synthesis step), then one lane of wave 0 (analysis) and one lane of wave 1 (synthesis)
// walk the tile: per frame the position of its first mark, the number of marks before it, and -- only where the frame
// holds a mark -- one ceiling division for its count (32-bit where the numerator fits, which it does for every hop below
// 65,536).  All lanes then expand the tile's marks in parallel: mark k finds its frame by a binary search over the tile's
// counts and is one multiply-add.  The carried state (position, count) lives in LDS between tiles.  After the last tile
// every synthesis mark finds its nearest analysis mark by a binary search over a (lower of two equally near ones) and
// reads its half width from the period table.  Loop bounds come from F, Lmax and the tile sizes; len is clamped to
// [0, Lmax] and every table value is clamped when read; nothing read from a table forms an address except a frame index
// that is clamped to [0, F).
//
// psola_ola_kernel: grid (tiles of 1,024 samples, B), 256 lanes, lane t owns samples t, t + 256, ... of the tile (adjacent
// lanes read adjacent source samples).  A grain reaches at most 1,023 samples either way, so the tile stages the grains
// with s in [tile start - 1023, last live sample + 1023] -- at most 192 of them, marks being 16 samples apart at least --
// into LDS once; a staged grain whose s or src lies outside its range is given width 0 and covers nothing.
#include "vc_common.h"

namespace {

constexpr int NT_P = 256;               // lanes of the plan kernel
constexpr int TF = 1024;                // frames per tile of the plan kernel
constexpr int OT = 256;                 // lanes of the overlap-add kernel
constexpr int OV = 4;                   // samples per lane
constexpr int TILE = OT * OV;
constexpr int P_MIN = 16 << 16, P_MAX = 1024 << 16, S_MAX = 2048 << 16;
constexpr int R_MIN = 32768, R_MAX = 131072;
constexpr int H_MIN = 16, H_MAX = 1024, REACH = H_MAX - 1;
constexpr int WIN_N = 2048;
constexpr int GCAP = (TILE + 2 * REACH - 1) / 16 + 1;               // 192: marks are >= 16 samples apart
constexpr int MAX_LEN = 1 << 24, MAX_F = 1 << 20, MAX_HOP = 65536;
constexpr int MARK_STEPS = 22;          // binary search over at most 2^20 + 1 marks
constexpr int TILE_STEPS = 11;          // ... over at most 1,024 frames of a tile

__device__ __forceinline__ int clamp_period(int p) { return min(max(p, P_MIN), P_MAX); }

__device__ __forceinline__ int synth_step(int P, int r) {
    const int R = min(max(r, R_MIN), R_MAX);
    const long long s = (((long long)P << 16) + (R >> 1)) / R;
    return (int)min(max(s, (long long)P_MIN), (long long)S_MAX);
}

struct PlanArgs {
    const int32_t* period_q;            // [B, F]
    const int32_t* ratio_q;             // [B, F]
    const int32_t* len;                 // [B]
    int F, hop, Lmax, M;
    int32_t* n_a;                       // [B]
    int32_t* n_s;                       // [B]
    int32_t* a;                         // [B, M]
    int32_t* s;
    int32_t* src;
    int32_t* h;
};

__global__ void __launch_bounds__(NT_P)
psola_plan_kernel(const PlanArgs g) {
    __shared__ int step[2][TF];
    __shared__ int first[2][TF + 1];
    __shared__ long long pos0[2][TF];
    __shared__ long long carry_pos[2];
    __shared__ int carry_cnt[2];
    const int t = threadIdx.x, b = blockIdx.x;
    const int len = min(max(g.len[b], 0), g.Lmax);
    const long long lenQ = (long long)len << 16;
    const int half = g.hop >> 1;
    const int nF = len > 0 ? min(g.F, (len - 1 + half) / g.hop + 1) : 0;        // the frames that hold a sample
    const int32_t* per = g.period_q + (size_t)b * g.F;
    const int32_t* rat = g.ratio_q + (size_t)b * g.F;
    const size_t row = (size_t)b * g.M;
    int32_t* const marks[2] = {g.a + row, g.s + row};
    if (t < 2) { carry_pos[t] = 0; carry_cnt[t] = 0; }
    __syncthreads();
    for (int f0 = 0; f0 < nF; f0 += TF) {
        const int tn = min(TF, nF - f0);
        for (int i = t; i < tn; i += NT_P) {
            const int P = clamp_period(per[f0 + i]);
            step[0][i] = P;
            step[1][i] = synth_step(P, rat[f0 + i]);
        }
        __syncthreads();
        if (t == 0 || t == 64) {
            const int w = t >> 6;
            long long p = carry_pos[w];
            int cnt = carry_cnt[w];
            for (int i = 0; i < tn; ++i) {
                const int f = f0 + i;
                const long long E = f == g.F - 1 ? lenQ : min(((long long)(f + 1) * g.hop - half) << 16, lenQ);
                first[w][i] = cnt;
                pos0[w][i] = p;
                if (p < E) {
                    const int T = step[w][i];
                    const unsigned long long num = (unsigned long long)(E - p) + (unsigned)(T - 1);
                    long long c = (num >> 32) == 0 ? (long long)((unsigned)num / (unsigned)T) : (long long)(num / (unsigned)T);
                    c = min(c, (long long)(g.M - cnt));             // (never less: marks are >= 16 samples apart)
                    cnt += (int)c;
                    p += c * T;
                }
            }
            first[w][tn] = cnt;
            carry_pos[w] = p;
            carry_cnt[w] = cnt;
        }
        __syncthreads();
        for (int w = 0; w < 2; ++w) {
            const int k1 = min(first[w][tn], g.M);
            for (int k = first[w][0] + t; k < k1; k += NT_P) {
                int lo = 0, hi = tn - 1;                            // the last frame of the tile whose count is <= k
                for (int it = 0; it < TILE_STEPS && lo < hi; ++it) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (first[w][mid] <= k) lo = mid; else hi = mid - 1;
                }
                marks[w][k] = (int)((pos0[w][lo] + (long long)(k - first[w][lo]) * step[w][lo]) >> 16);
            }
        }
        __syncthreads();                                            // the tile's tables, before the next one overwrites them
    }
    const int K = min(carry_cnt[0], g.M), J = min(carry_cnt[1], g.M);
    if (t == 0) { g.n_a[b] = K; g.n_s[b] = J; }
    const int32_t* a = g.a + row;
    const int32_t* s = g.s + row;
    for (int k = K + t; k < g.M; k += NT_P) g.a[row + k] = -1;
    for (int j = t; j < g.M; j += NT_P) {
        int sv = -1, src = -1, hh = -1;
        if (j < J) {
            sv = s[j];
            int lo = 0, hi = K;                                     // the first analysis mark at or after s_j
            for (int it = 0; it < MARK_STEPS && lo < hi; ++it) {
                const int mid = (lo + hi) >> 1;
                if (a[mid] < sv) lo = mid + 1; else hi = mid;
            }
            int k = lo;
            if (k >= K) k = K - 1;
            else if (k > 0 && sv - a[k - 1] <= a[k] - sv) k = k - 1;
            src = a[k];
            const int f = min(max((src + half) / g.hop, 0), g.F - 1);
            hh = (clamp_period(per[f]) + 32768) >> 16;
        }
        if (j >= J) g.s[row + j] = sv;
        g.src[row + j] = src;
        g.h[row + j] = hh;
    }
}

// one covering grain: two separately rounded operations for N, one for D (no contraction)
__device__ __forceinline__ void accumulate_rn(float& N, float& D, float xv, float w) {
#pragma clang fp contract(off)
    const float m = xv * w;
    N = N + m;
    D = D + w;
}

__global__ void __launch_bounds__(OT)
psola_ola_kernel(const float* __restrict__ x, const int32_t* __restrict__ len_all, const int32_t* __restrict__ n_s_all,
                 const int32_t* __restrict__ s_all, const int32_t* __restrict__ src_all, const int32_t* __restrict__ h_all,
                 const float* __restrict__ W, int Lmax, int M, float w_floor, float* __restrict__ y) {
    __shared__ int gs[GCAP], gsrc[GCAP], gh[GCAP];
    const int t = threadIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.x * TILE;
    const int len = min(max(len_all[b], 0), Lmax);
    float* yb = y + (size_t)b * Lmax;
    if (t0 >= len) {
#pragma unroll
        for (int v = 0; v < OV; ++v) {
            const int n = t0 + t + v * OT;
            if (n < Lmax) yb[n] = 0.0f;
        }
        return;
    }
    const float* xb = x + (size_t)b * Lmax;
    const size_t row = (size_t)b * M;
    const int32_t* s = s_all + row;
    const int J = min(max(n_s_all[b], 0), M);
    const int lo_s = t0 - REACH, hi_s = min(t0 + TILE, len) - 1 + REACH;
    int j_lo = 0, j_hi = J;                                         // the first mark >= lo_s, the first mark > hi_s
    {
        int hi = J;
        for (int it = 0; it < MARK_STEPS && j_lo < hi; ++it) {
            const int mid = (j_lo + hi) >> 1;
            if (s[mid] < lo_s) j_lo = mid + 1; else hi = mid;
        }
        int lo = j_lo;
        for (int it = 0; it < MARK_STEPS && lo < j_hi; ++it) {
            const int mid = (lo + j_hi) >> 1;
            if (s[mid] <= hi_s) lo = mid + 1; else j_hi = mid;
        }
    }
    const int n_g = min(max(j_hi - j_lo, 0), GCAP);
    for (int i = t; i < n_g; i += OT) {
        const int sv = s[j_lo + i], sr = src_all[row + j_lo + i];
        const bool ok = sv >= lo_s && sv <= hi_s && sr >= 0 && sr < len;
        gs[i] = ok ? sv : 0;
        gsrc[i] = ok ? sr : 0;
        gh[i] = ok ? min(max(h_all[row + j_lo + i], H_MIN), H_MAX) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < OV; ++v) {
        const int n = t0 + t + v * OT;
        if (n >= Lmax) break;
        float N = 0.0f, D = 0.0f;
        if (n < len) {
            for (int i = 0; i < n_g; ++i) {
                const int d = n - gs[i], hh = gh[i];
                const int ad = d < 0 ? -d : d;
                if (ad < hh) {
                    const int idx = min((ad * WIN_N + (hh >> 1)) / hh, WIN_N);
                    const int m = gsrc[i] + d;
                    const float xv = (m >= 0 && m < len) ? xb[m] : 0.0f;
                    accumulate_rn(N, D, xv, W[idx]);
                }
            }
        }
        yb[n] = n < len ? N / fmaxf(D, w_floor) : 0.0f;
    }
}

inline bool pitch_shape_ok(int batch, int max_len) { return batch <= 65535 && max_len <= MAX_LEN; }

}  // namespace

extern "C" {

int32_t vc_psola_max_marks(int32_t max_len) {
    return max_len >= 1 && max_len <= MAX_LEN ? max_len / 16 + 1 : 0;
}

int vc_psola_plan(const int32_t* d_period_q, const int32_t* d_ratio_q, const int32_t* d_len, int32_t batch, int32_t max_len,
                  int32_t n_frames, int32_t hop, int32_t* d_n_a, int32_t* d_n_s, int32_t* d_a, int32_t* d_s, int32_t* d_src,
                  int32_t* d_h, void* stream) {
    VC_REQUIRE(d_period_q && d_ratio_q && d_len && d_n_a && d_n_s && d_a && d_s && d_src && d_h, "vc_psola_plan: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1 && n_frames >= 1 && hop >= 1, "vc_psola_plan: bad shape (batch %d, max_len %d, "
               "n_frames %d, hop %d)", batch, max_len, n_frames, hop);
    if (!pitch_shape_ok(batch, max_len) || n_frames > MAX_F || hop > MAX_HOP)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_psola_plan: limits are batch <= 65535, max_len <= %d, n_frames <= %d and "
                             "hop <= %d; got batch %d, max_len %d, n_frames %d, hop %d", MAX_LEN, MAX_F, MAX_HOP, batch, max_len,
                             n_frames, hop);
    PlanArgs g;
    g.period_q = d_period_q; g.ratio_q = d_ratio_q; g.len = d_len; g.F = n_frames; g.hop = hop; g.Lmax = max_len;
    g.M = vc_psola_max_marks(max_len); g.n_a = d_n_a; g.n_s = d_n_s; g.a = d_a; g.s = d_s; g.src = d_src; g.h = d_h;
    hipLaunchKernelGGL(psola_plan_kernel, dim3(batch), dim3(NT_P), 0, static_cast<hipStream_t>(stream), g);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_psola_ola_f32(const float* d_x, const int32_t* d_len, const int32_t* d_n_s, const int32_t* d_s, const int32_t* d_src,
                     const int32_t* d_h, const float* d_window, int32_t batch, int32_t max_len, float w_floor, float* d_y,
                     void* stream) {
    VC_REQUIRE(d_x && d_len && d_n_s && d_s && d_src && d_h && d_window && d_y, "vc_psola_ola_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1, "vc_psola_ola_f32: bad shape (batch %d, max_len %d)", batch, max_len);
    VC_REQUIRE(w_floor > 0.0f && w_floor <= 3.0e38f, "vc_psola_ola_f32: w_floor must be positive and finite");
    VC_REQUIRE(d_x != d_y, "vc_psola_ola_f32: not in place");
    if (!pitch_shape_ok(batch, max_len))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_psola_ola_f32: limits are batch <= 65535 and max_len <= %d; got batch %d, "
                             "max_len %d", MAX_LEN, batch, max_len);
    hipLaunchKernelGGL(psola_ola_kernel, dim3((max_len + TILE - 1) / TILE, batch), dim3(OT), 0, static_cast<hipStream_t>(stream),
                       d_x, d_len, d_n_s, d_s, d_src, d_h, d_window, max_len, vc_psola_max_marks(max_len), w_floor, d_y);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
