// Pitch on the device (include/vc_hip.h, "Evaluation"): the YIN F0 tracker and the F0 / voicing figures of a pair of
// tracks along a DTW path.
//
//     d(tau)   = sum_{j < W} (x[s + j] - x[s + j + tau])^2,  tau = 0 .. tau_max + 1          (the direct form)
//     d'(tau)  = d(tau) * tau / sum_{k = 1..tau} d(k),  d'(0) = 1,  1 where the sum is zero
//     tau      = the first lag in [tau_min, tau_max] below the threshold, walked on to the bottom of its dip
//     f0       = sr / (tau + parabola offset),  aperiodicity = min d' over [tau_min, tau_max]
//
// f0_yin_kernel: one workgroup per (utterance, tile of G consecutive frames).  The tile's samples are staged once in
// LDS (W + tau_max + 1 + (G - 1) hop floats), zeros outside [0, len).  Lane t owns lag t of every frame of the tile (the
// workgroup has tau_max + 2 lanes rounded up to whole waves): x[s + j] is one address for the whole wave (a broadcast),
// x[s + j + t] is consecutive over lanes -- 32 consecutive words fall on 32 different banks whatever s + j is.  One
// chain of fused multiply-adds per lag, j ascending.  The running sum over lags is a scan in a fixed order: Kogge-Stone
// inside a wave (six steps of lane t adding lane t - 2^k), then the totals of the waves before this one added in order.
// d' goes to LDS; the first lag below the threshold and the minimum are reductions (exact, whatever their order); lane 0
// walks to the bottom of the dip and fits the parabola.
//
// f0_candidates_kernel: the same tiling and the same d' (yin_stage, yin_dprime and yin_refine are the one text both kernels
// use), then every local minimum of d' below a ceiling instead of the first dip below a threshold; see the kernel.
//
// A frame's result depends on that utterance's samples alone and on nothing that varies from run to run: no atomics, no
// hand-off between workgroups, and G (chosen from the LDS budget) changes which workgroup computes a frame, not how.
//
// f0_metrics_kernel: one workgroup per pair, cells dealt to lanes by stride, partial sums added in a fixed tree.  The
// sums run in float64 (two logarithms and a handful of additions per cell): the figures are the float32 roundings of
// nearly exact values, and the correlation is taken about the means (a second pass over the cells), not from raw moments.
#include <cmath>
#include "vc_common.h"

namespace {

constexpr int MAX_W = 2048;             // integration length
constexpr int MAX_LAGS = 1024;          // tau_max + 2 lags, one per lane
constexpr int MAX_HOP = 65536;
constexpr int MAX_SAMPLES = 1 << 30;    // f * hop and every sample index stay in int32
constexpr int MAX_CELLS = 1 << 30;
constexpr int LDS_BUDGET = 64 * 1024;   // the default limit: no function attribute, capturable from the first call
constexpr int NT_M = 256;               // lanes of the metrics kernel
constexpr int MAX_CAND = 15;            // candidates per frame: with the unvoiced state, 16 states (csrc/vc_f0_track.hip)

inline int yin_lanes(int tau_max) { return (tau_max + 2 + 63) & ~63; }
inline size_t yin_lds_bytes(int W, int tau_max, int hop, int G) {
    return ((size_t)W + tau_max + 1 + (size_t)(G - 1) * hop + yin_lanes(tau_max) + 64) * sizeof(float);
}
inline size_t cand_lds_bytes(int W, int tau_max, int hop, int G) { return yin_lds_bytes(W, tau_max, hop, G) + 64 * sizeof(float); }

// The tile's samples, zeros outside [0, len): xs[e] = x[s0 + e], e < n_stage.
__device__ __forceinline__ void yin_stage(float* xs, const float* __restrict__ x, int s0, int n_stage, int len, int t, int NT) {
    for (int e = t; e < n_stage; e += NT) {
        const int i = s0 + e;
        xs[e] = (i >= 0 && i < len) ? x[i] : 0.0f;
    }
}

// d'(t) of the frame at `a`, also left in dp[t]: the difference, the scan and the normalisation, shared by f0_yin_kernel
// and f0_candidates_kernel (one text, so both see the same d' bit for bit).  Holds one __syncthreads().
__device__ __forceinline__ float yin_dprime(const float* a, int W, int n_lags, int t, int lane, int wave, float* dp, float* wtot) {
    // lanes beyond the last lag repeat it (their reads stay inside the stage) and are left out below
    const float* c = a + min(t, n_lags - 1);
    float acc = 0.0f;
    int j = 0;
    for (; j + 8 <= W; j += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float df = a[j + u] - c[j + u];
            acc = fmaf(df, df, acc);
        }
    }
    for (; j < W; ++j) {
        const float df = a[j] - c[j];
        acc = fmaf(df, df, acc);
    }
    const float d = t < n_lags ? acc : 0.0f;
    float v = d;                                                    // inclusive scan over lags; d(0) is exactly zero
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float u = __shfl_up(v, s, 64);
        if (lane >= s) v += u;
    }
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    float off = 0.0f;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    const float S = wave == 0 ? v : v + off;
    float q = 1.0f;
    if (t > 0 && S > 0.0f) q = (d * (float)t) / S;
    dp[t] = q;
    return q;
}

// f0 of the dip at lag tau: the clamped parabola through d'(tau - 1 .. tau + 1)
__device__ __forceinline__ float yin_refine(const float* dp, int tau, float sr) {
    const float y0 = dp[tau - 1], y1 = dp[tau], y2 = dp[tau + 1];
    const float den = (y0 - 2.0f * y1) + y2;
    float o = den > 0.0f ? 0.5f * (y0 - y2) / den : 0.0f;
    o = fminf(fmaxf(o, -0.5f), 0.5f);
    return sr / ((float)tau + o);
}

__global__ void __launch_bounds__(MAX_LAGS)
f0_yin_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, int max_len, int ld, float sr, int hop, int W,
              int tau_min, int tau_max, float threshold, int G, float* __restrict__ f0, float* __restrict__ aper,
              int max_frames) {
    extern __shared__ __align__(16) float lds[];
    const int t = threadIdx.x;
    const int NT = blockDim.x;
    const int lane = t & 63, wave = t >> 6, n_waves = NT >> 6;
    const int n_lags = tau_max + 2;
    const int span = W + tau_max + 1;                               // samples one frame reads
    const int n_stage = span + (G - 1) * hop;
    float* xs = lds;                                                // [n_stage]
    float* dp = xs + n_stage;                                       // [NT]: d' of the frame in hand
    float* wtot = dp + NT;                                          // [16] totals of the waves' scans
    float* wmin = wtot + 16;                                        // [16] minima of d'
    int* wfirst = reinterpret_cast<int*>(wmin + 16);                // [16] first lags below the threshold
    const int b = blockIdx.y;
    const int g0 = blockIdx.x * G;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    const int n_fr = 1 + len / hop;
    float* out_f = f0 + (size_t)b * max_frames;
    float* out_a = aper + (size_t)b * max_frames;
    const int g_end = min(g0 + G, max_frames);
    if (g0 >= n_fr) {                                               // the whole tile lies beyond the utterance
        for (int f = g0 + t; f < g_end; f += NT) { out_f[f] = 0.0f; out_a[f] = 1.0f; }
        return;
    }
    yin_stage(xs, wav + (size_t)b * ld, g0 * hop - (W + tau_max) / 2, n_stage, len, t, NT);
    __syncthreads();
    for (int f = g0; f < g_end; ++f) {
        if (f >= n_fr) {                                            // uniform over the workgroup
            if (t == 0) { out_f[f] = 0.0f; out_a[f] = 1.0f; }
            continue;
        }
        const float q = yin_dprime(xs + (f - g0) * hop, W, n_lags, t, lane, wave, dp, wtot);
        const bool in_range = t >= tau_min && t <= tau_max;
        float m = in_range ? q : __builtin_inff();
        int first = (in_range && q < threshold) ? t : 0x7fffffff;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            m = fminf(m, __shfl_xor(m, s, 64));
            first = min(first, __shfl_xor(first, s, 64));
        }
        if (lane == 0) { wmin[wave] = m; wfirst[wave] = first; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < n_waves; ++w) { m = fminf(m, wmin[w]); first = min(first, wfirst[w]); }
            float hz = 0.0f;
            if (first <= tau_max) {
                int tau = first;
                while (tau + 1 <= tau_max && dp[tau + 1] < dp[tau]) ++tau;
                hz = yin_refine(dp, tau, sr);
            }
            out_f[f] = hz;
            out_a[f] = m;
        }
        __syncthreads();                                            // dp, wtot, wmin and wfirst are written again by the next frame
    }
}

// The candidates of every frame (include/vc_hip.h, "Pitch tracking"): f0_yin_kernel's tiling, staging and d', then the
// local minima of d' below the ceiling, the n_cand lowest of them by repeated arg-min over (d', lag), written in
// ascending lag.  A round of the selection: each wave's minimum on DPP, the lowest lane that holds it from a ballot (lags
// ascend with lanes, so that is the smallest lag), the waves' pairs through LDS (two buffers in turn: one barrier a
// round), every lane scanning them in wave order with a strict compare, so the smaller lag wins a tie.  The chosen
// lanes then count the chosen lanes below them (a ballot and the waves' counts), refine their own lag and store it.
__global__ void __launch_bounds__(MAX_LAGS)
f0_candidates_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, int max_len, int ld, float sr, int hop, int W,
                     int tau_min, int tau_max, float ceiling, int n_cand, int G, float* __restrict__ c_f0,
                     float* __restrict__ c_pitch, float* __restrict__ c_cost, int32_t* __restrict__ c_n, float* __restrict__ aper,
                     int max_frames) {
    extern __shared__ __align__(16) float lds[];
    const int t = threadIdx.x;
    const int NT = blockDim.x;
    const int lane = t & 63, wave = t >> 6, n_waves = NT >> 6;
    const int n_lags = tau_max + 2;
    const int n_stage = W + tau_max + 1 + (G - 1) * hop;
    float* xs = lds;                                                // [n_stage]
    float* dp = xs + n_stage;                                       // [NT]
    float* wtot = dp + NT;                                          // [16]
    float* wmin = wtot + 16;                                        // [16]
    float* wkq = wmin + 16;                                         // [2][16] the waves' lowest d' of a round
    int* wkt = reinterpret_cast<int*>(wkq + 32);                    // [2][16] and its lag
    int* wcnt = wkt + 32;                                           // [16] chosen lanes per wave
    const float NONE = 3.402823466e38f;                             // vc::wave_min's identity; no candidate holds it (d' < ceiling)
    const int b = blockIdx.y;
    const int g0 = blockIdx.x * G;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    const int n_fr = 1 + len / hop;
    const size_t row = (size_t)b * max_frames;
    const int g_end = min(g0 + G, max_frames);
    if (g0 >= n_fr) {                                               // the whole tile lies beyond the utterance
        for (int f = g0 + t; f < g_end; f += NT) { c_n[row + f] = 0; aper[row + f] = 1.0f; }
        const size_t e0 = (row + g0) * n_cand, e1 = (row + g_end) * n_cand;
        for (size_t e = e0 + t; e < e1; e += NT) { c_f0[e] = 0.0f; c_pitch[e] = 0.0f; c_cost[e] = 1.0f; }
        return;
    }
    yin_stage(xs, wav + (size_t)b * ld, g0 * hop - (W + tau_max) / 2, n_stage, len, t, NT);
    __syncthreads();
    for (int f = g0; f < g_end; ++f) {
        const size_t o = (row + f) * n_cand;
        if (f >= n_fr) {                                            // uniform over the workgroup
            if (t < n_cand) { c_f0[o + t] = 0.0f; c_pitch[o + t] = 0.0f; c_cost[o + t] = 1.0f; }
            if (t == 0) { c_n[row + f] = 0; aper[row + f] = 1.0f; }
            continue;
        }
        const float q = yin_dprime(xs + (f - g0) * hop, W, n_lags, t, lane, wave, dp, wtot);
        const bool in_range = t >= tau_min && t <= tau_max;
        float m = in_range ? q : __builtin_inff();
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) m = fminf(m, __shfl_xor(m, s, 64));
        if (lane == 0) wmin[wave] = m;
        __syncthreads();                                            // every d' is in dp
        const bool flag = in_range && q < ceiling && (t == tau_min || q < dp[t - 1]) && (t == tau_max || q <= dp[t + 1]);
        float key = flag ? q : NONE;
        bool taken = false;
        for (int k = 0; k < n_cand; ++k) {
            const float wm = vc::wave_min(key);
            const unsigned long long held = __ballot(key == wm);
            if (lane == 0) {
                wkq[(k & 1) * 16 + wave] = wm;
                wkt[(k & 1) * 16 + wave] = wm < NONE ? (wave << 6) + __ffsll((long long)held) - 1 : 0x7fffffff;
            }
            __syncthreads();
            float bq = NONE;
            int bt = 0x7fffffff;
            for (int w = 0; w < n_waves; ++w) {
                const float wq = wkq[(k & 1) * 16 + w];
                if (wq < bq) { bq = wq; bt = wkt[(k & 1) * 16 + w]; }
            }
            if (bt == 0x7fffffff) break;                            // uniform: no local minimum is left
            if (t == bt) { taken = true; key = NONE; }
        }
        const unsigned long long chosen = __ballot(taken);
        if (lane == 0) wcnt[wave] = __popcll(chosen);
        __syncthreads();
        int below = __popcll(chosen & ((1ull << lane) - 1ull)), n = 0;
        for (int w = 0; w < n_waves; ++w) {
            const int c = wcnt[w];
            if (w < wave) below += c;
            n += c;
        }
        if (taken) {
            const float hz = yin_refine(dp, t, sr);
            c_f0[o + below] = hz;
            c_pitch[o + below] = log2f(hz);
            c_cost[o + below] = q;
        }
        if (t >= n && t < n_cand) { c_f0[o + t] = 0.0f; c_pitch[o + t] = 0.0f; c_cost[o + t] = 1.0f; }
        if (t == 0) {
            for (int w = 1; w < n_waves; ++w) m = fminf(m, wmin[w]);
            c_n[row + f] = n;
            aper[row + f] = m;
        }
        __syncthreads();                                            // dp and the waves' words are written again by the next frame
    }
}

// sum of v over the workgroup in a fixed tree, in every lane
__device__ inline double block_sum(double v, double* buf) {
    const int t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int w = NT_M / 2; w > 0; w >>= 1) {
        if (t < w) buf[t] += buf[t + w];
        __syncthreads();
    }
    return buf[0];
}

// minimum of v over the workgroup, in every lane
__device__ inline double block_min(double v, double* buf) {
    const int t = threadIdx.x;
    __syncthreads();
    buf[t] = v;
    __syncthreads();
    for (int w = NT_M / 2; w > 0; w >>= 1) {
        if (t < w) buf[t] = fmin(buf[t], buf[t + w]);
        __syncthreads();
    }
    return buf[0];
}

// path [batch, max_path, 2] with path_len [batch], or NULL: cells (i, i), i < min(len_a, len_b).
// counts [batch, 3]: n_cells, n_both_voiced, n_vuv_mismatch.  values [batch, 4]: vuv_error, rmse cents, rmse Hz, corr.
__global__ void __launch_bounds__(NT_M)
f0_metrics_kernel(const float* __restrict__ f0_a, const float* __restrict__ f0_b, const int32_t* __restrict__ len_a,
                  const int32_t* __restrict__ len_b, int max_a, int max_b, const int32_t* __restrict__ path,
                  const int32_t* __restrict__ path_len, int max_path, int32_t* __restrict__ counts, float* __restrict__ values) {
    __shared__ double buf[NT_M];
    const int p = blockIdx.x;
    const int t = threadIdx.x;
    const int la = min(max(len_a[p], 1), max_a);
    const int lb = min(max(len_b[p], 1), max_b);
    const float* __restrict__ A = f0_a + (size_t)p * max_a;
    const float* __restrict__ B = f0_b + (size_t)p * max_b;
    const int32_t* __restrict__ P = path ? path + (size_t)p * max_path * 2 : nullptr;
    const int n = path ? min(max(path_len[p], 0), max_path) : min(la, lb);
    const double INF = __builtin_inf();
    double cells = 0.0, both = 0.0, mism = 0.0, c2 = 0.0, hz2 = 0.0, sa = 0.0, sb = 0.0;
    double lo_a = INF, hi_a = -INF, lo_b = INF, hi_b = -INF;
    for (int k = t; k < n; k += NT_M) {
        const int i = P ? P[2 * k] : k, j = P ? P[2 * k + 1] : k;
        if (i < 0 || i >= la || j < 0 || j >= lb) continue;
        const float fa = A[i], fb = B[j];
        const bool va = fa > 0.0f, vb = fb > 0.0f;
        cells += 1.0;
        if (va != vb) mism += 1.0;
        if (va && vb) {
            const double xa = log2((double)fa), xb = log2((double)fb);
            const double c = 1200.0 * log2((double)fa / (double)fb), h = (double)fa - (double)fb;
            both += 1.0;
            c2 += c * c;
            hz2 += h * h;
            sa += xa;
            sb += xb;
            lo_a = fmin(lo_a, xa); hi_a = fmax(hi_a, xa);
            lo_b = fmin(lo_b, xb); hi_b = fmax(hi_b, xb);
        }
    }
    cells = block_sum(cells, buf);                                  // counts below 2^53 are exact in float64
    both = block_sum(both, buf);
    mism = block_sum(mism, buf);
    c2 = block_sum(c2, buf);
    hz2 = block_sum(hz2, buf);
    sa = block_sum(sa, buf);
    sb = block_sum(sb, buf);
    lo_a = block_min(lo_a, buf);
    hi_a = -block_min(-hi_a, buf);
    lo_b = block_min(lo_b, buf);
    hi_b = -block_min(-hi_b, buf);
    const bool corr_ok = both >= 2.0 && lo_a < hi_a && lo_b < hi_b;
    double saa = 0.0, sbb = 0.0, sab = 0.0;
    if (corr_ok) {                                                  // uniform over the workgroup
        const double ma = sa / both, mb = sb / both;
        for (int k = t; k < n; k += NT_M) {
            const int i = P ? P[2 * k] : k, j = P ? P[2 * k + 1] : k;
            if (i < 0 || i >= la || j < 0 || j >= lb) continue;
            const float fa = A[i], fb = B[j];
            if (fa > 0.0f && fb > 0.0f) {
                const double xa = log2((double)fa) - ma, xb = log2((double)fb) - mb;
                saa += xa * xa;
                sbb += xb * xb;
                sab += xa * xb;
            }
        }
        saa = block_sum(saa, buf);
        sbb = block_sum(sbb, buf);
        sab = block_sum(sab, buf);
    }
    if (t == 0) {
        const float nan = __builtin_nanf("");
        counts[3 * p] = (int32_t)cells;
        counts[3 * p + 1] = (int32_t)both;
        counts[3 * p + 2] = (int32_t)mism;
        values[4 * p] = cells > 0.0 ? (float)(mism / cells) : nan;
        values[4 * p + 1] = both > 0.0 ? (float)sqrt(c2 / both) : nan;
        values[4 * p + 2] = both > 0.0 ? (float)sqrt(hz2 / both) : nan;
        values[4 * p + 3] = corr_ok ? (float)(sab / sqrt(saa * sbb)) : nan;
    }
}

}  // namespace

extern "C" {

int vc_f0_yin_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, float sample_rate,
                  int32_t hop, int32_t frame_length, int32_t tau_min, int32_t tau_max, float threshold, float* d_f0,
                  float* d_aperiodicity, int32_t max_frames, void* stream) {
    VC_REQUIRE(d_wav && d_f0 && d_aperiodicity, "vc_f0_yin_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1 && ld >= max_len && hop >= 1 && frame_length >= 1,
               "vc_f0_yin_f32: bad shape (batch %d, max_len %d, ld %d, hop %d, frame_length %d; need all >= 1 and ld >= max_len)", batch,
               max_len, ld, hop, frame_length);
    VC_REQUIRE(tau_min >= 1 && tau_max >= tau_min, "vc_f0_yin_f32: need 1 <= tau_min <= tau_max (got %d, %d)", tau_min, tau_max);
    VC_REQUIRE(std::isfinite(sample_rate) && sample_rate > 0.0f && std::isfinite(threshold) && threshold > 0.0f && threshold <= 1.0f,
               "vc_f0_yin_f32: need a finite sample_rate > 0 and 0 < threshold <= 1 (got %g, %g)", (double)sample_rate, (double)threshold);
    VC_REQUIRE(max_frames >= 1, "vc_f0_yin_f32: max_frames must be at least 1 (got %d)", max_frames);
    if (batch > 65535 || max_len > MAX_SAMPLES || frame_length > MAX_W || tau_max + 2 > MAX_LAGS || hop > MAX_HOP ||
        max_frames > MAX_SAMPLES + 1)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_f0_yin_f32: limits are batch <= 65535, max_len <= %d, frame_length <= %d, tau_max <= %d "
                             "(one lane per lag), hop <= %d, max_frames <= %d; got batch %d, max_len %d, frame_length %d, tau_max %d, hop %d, "
                             "max_frames %d", MAX_SAMPLES, MAX_W, MAX_LAGS - 2, MAX_HOP, MAX_SAMPLES + 1, batch, max_len, frame_length,
                             tau_max, hop, max_frames);
    VC_REQUIRE(max_frames >= 1 + max_len / hop, "vc_f0_yin_f32: max_frames %d is less than 1 + max_len / hop = %d", max_frames,
               1 + max_len / hop);
    int G = 16;                                                     // frames per tile: the most the default LDS limit holds
    while (G > 1 && yin_lds_bytes(frame_length, tau_max, hop, G) > (size_t)LDS_BUDGET) G >>= 1;
    const dim3 grid((unsigned)((max_frames + G - 1) / G), (unsigned)batch);
    hipLaunchKernelGGL(f0_yin_kernel, grid, dim3(yin_lanes(tau_max)), yin_lds_bytes(frame_length, tau_max, hop, G),
                       static_cast<hipStream_t>(stream), d_wav, d_lens, max_len, ld, sample_rate, hop, frame_length, tau_min, tau_max,
                       threshold, G, d_f0, d_aperiodicity, max_frames);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_f0_candidates_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, float sample_rate,
                         int32_t hop, int32_t frame_length, int32_t tau_min, int32_t tau_max, float ceiling, int32_t n_cand,
                         float* d_f0, float* d_pitch, float* d_cost, int32_t* d_n, float* d_aperiodicity, int32_t max_frames,
                         void* stream) {
    VC_REQUIRE(d_wav && d_f0 && d_pitch && d_cost && d_n && d_aperiodicity, "vc_f0_candidates_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1 && ld >= max_len && hop >= 1 && frame_length >= 1 && n_cand >= 1,
               "vc_f0_candidates_f32: bad shape (batch %d, max_len %d, ld %d, hop %d, frame_length %d, n_cand %d; need all >= 1 and "
               "ld >= max_len)", batch, max_len, ld, hop, frame_length, n_cand);
    VC_REQUIRE(tau_min >= 1 && tau_max >= tau_min, "vc_f0_candidates_f32: need 1 <= tau_min <= tau_max (got %d, %d)", tau_min, tau_max);
    VC_REQUIRE(std::isfinite(sample_rate) && sample_rate > 0.0f && std::isfinite(ceiling) && ceiling > 0.0f,
               "vc_f0_candidates_f32: need a finite sample_rate > 0 and a finite ceiling > 0 (got %g, %g)", (double)sample_rate,
               (double)ceiling);
    VC_REQUIRE(max_frames >= 1, "vc_f0_candidates_f32: max_frames must be at least 1 (got %d)", max_frames);
    if (batch > 65535 || max_len > MAX_SAMPLES || frame_length > MAX_W || tau_max + 2 > MAX_LAGS || hop > MAX_HOP ||
        max_frames > MAX_SAMPLES + 1 || n_cand > MAX_CAND)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_f0_candidates_f32: limits are batch <= 65535, max_len <= %d, frame_length <= %d, "
                             "tau_max <= %d (one lane per lag), hop <= %d, max_frames <= %d, n_cand <= %d; got batch %d, max_len %d, "
                             "frame_length %d, tau_max %d, hop %d, max_frames %d, n_cand %d", MAX_SAMPLES, MAX_W, MAX_LAGS - 2, MAX_HOP,
                             MAX_SAMPLES + 1, MAX_CAND, batch, max_len, frame_length, tau_max, hop, max_frames, n_cand);
    VC_REQUIRE(max_frames >= 1 + max_len / hop, "vc_f0_candidates_f32: max_frames %d is less than 1 + max_len / hop = %d", max_frames,
               1 + max_len / hop);
    int G = 16;
    while (G > 1 && cand_lds_bytes(frame_length, tau_max, hop, G) > (size_t)LDS_BUDGET) G >>= 1;
    const dim3 grid((unsigned)((max_frames + G - 1) / G), (unsigned)batch);
    hipLaunchKernelGGL(f0_candidates_kernel, grid, dim3(yin_lanes(tau_max)), cand_lds_bytes(frame_length, tau_max, hop, G),
                       static_cast<hipStream_t>(stream), d_wav, d_lens, max_len, ld, sample_rate, hop, frame_length, tau_min, tau_max,
                       ceiling, n_cand, G, d_f0, d_pitch, d_cost, d_n, d_aperiodicity, max_frames);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_f0_metrics_f32(const float* d_f0_a, const float* d_f0_b, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
                      int32_t max_a, int32_t max_b, const int32_t* d_path, const int32_t* d_path_len, int32_t max_path,
                      int32_t* d_counts, float* d_values, void* stream) {
    VC_REQUIRE(d_f0_a && d_f0_b && d_len_a && d_len_b && d_counts && d_values, "vc_f0_metrics_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_a >= 1 && max_b >= 1, "vc_f0_metrics_f32: bad shape (batch %d, max_a %d, max_b %d)", batch, max_a, max_b);
    VC_REQUIRE((d_path == nullptr) == (d_path_len == nullptr) && (d_path ? max_path >= 1 : max_path == 0),
               "vc_f0_metrics_f32: pass d_path, d_path_len and max_path >= 1 together, or NULL, NULL and 0 (max_path %d)", max_path);
    if (batch > 65535 || max_a > MAX_CELLS || max_b > MAX_CELLS || max_path > MAX_CELLS)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_f0_metrics_f32: limits are batch <= 65535 and max_a, max_b, max_path <= %d; got batch "
                             "%d, max_a %d, max_b %d, max_path %d", MAX_CELLS, batch, max_a, max_b, max_path);
    hipLaunchKernelGGL(f0_metrics_kernel, dim3(batch), dim3(NT_M), 0, static_cast<hipStream_t>(stream), d_f0_a, d_f0_b, d_len_a,
                       d_len_b, max_a, max_b, d_path, d_path_len, max_path, d_counts, d_values);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
