// Speech activity on the device (include/vc_hip.h, "Evaluation"): frame energy, the per-utterance mask with its two
// run-length smoothing passes, the compaction of a mask into a list of frames and intervals, the gather of rows by
// that list, and the map of a DTW path over compacted frames back to the original frame numbers.
//
//     e[f]   = sum_{j < W} x[s + j]^2,  s = f * hop - W / 2, zeros outside [0, len),  F = 1 + len / hop frames
//     raw    = e > 0 and e > float32(ratio * max_f e)   ('energy'),  f0 > 0  ('voiced'),  or both
//     smooth = gaps of at most max_gap frames between two active frames filled, then runs shorter than min_run dropped
//
// frame_energy_kernel: one workgroup per (utterance, tile of G consecutive frames).  The tile's W + (G - 1) hop samples
// are staged once in LDS; one wave per frame: lane l adds the squares of samples l, l + 64, l + 128, ... of the frame in
// that order (one chain of fused multiply-adds; the 64 lanes read 64 consecutive words, which fall on different banks
// whatever the frame's offset is), then the 64 partial sums are added in a butterfly (lane l adds lane l ^ 32, then
// l ^ 16, ... l ^ 1: the same tree in every lane).  Which wave or tile a frame lands in changes nothing in its sum.
//
// activity_mask_kernel and mask_compact_kernel: one workgroup of 1,024 lanes per utterance, lane t owns the frames
// [t * C, (t + 1) * C), C = ceil(F / 1024) <= 16.  Everything after the threshold is integer work: the index of the
// previous / next frame of a kind is a max / min scan over the lanes' chunks, the position of a frame in the compacted
// list a sum scan (Hillis-Steele in LDS, a fixed order).  No atomics, no hand-off between workgroups, no workspace.
//
// speech_gain_kernel / scale_rows_kernel: the front-end's amplitude normalisation taken over the speech samples only, so that
// a masked score does not depend on how much silence a recording carries (include/vc_hip.h).
#include <cmath>
#include "vc_common.h"

namespace {

constexpr int MAX_FRAMES = 16384;       // vc_dtw_f32's limit
constexpr int MAX_W = 8192;
constexpr int MAX_HOP = 65536;
constexpr int MAX_SAMPLES = 1 << 30;    // f * hop and every sample index stay in int32
constexpr int MAX_COLS = 4096;
constexpr int LDS_BUDGET = 64 * 1024;   // the default limit: no function attribute, capturable from the first call
constexpr int NT_E = 256;               // lanes of the energy kernel: four waves, a frame each
constexpr int NT_U = 1024;              // lanes of the per-utterance kernels
constexpr int NT_G = 256;

inline size_t energy_lds_bytes(int W, int hop, int G) { return ((size_t)W + (size_t)(G - 1) * hop) * sizeof(float); }
inline int energy_tile(int W, int hop) {
    int G = 64;
    while (G > 1 && energy_lds_bytes(W, hop, G) > (size_t)LDS_BUDGET) G >>= 1;
    return G;
}

__global__ void __launch_bounds__(NT_E)
frame_energy_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, int max_len, int ld, int hop, int W, int G,
                    float* __restrict__ energy, int max_frames) {
    extern __shared__ __align__(16) float xs[];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int b = blockIdx.y;
    const int g0 = blockIdx.x * G;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    const int n_fr = 1 + len / hop;
    float* out = energy + (size_t)b * max_frames;
    const int g_end = min(g0 + G, max_frames);
    if (g0 >= n_fr) {                                               // the whole tile lies beyond the utterance
        for (int f = g0 + t; f < g_end; f += NT_E) out[f] = 0.0f;
        return;
    }
    const float* __restrict__ x = wav + (size_t)b * ld;
    const int n_stage = W + (G - 1) * hop;
    const int s0 = g0 * hop - W / 2;
    for (int e = t; e < n_stage; e += NT_E) {
        const int i = s0 + e;
        xs[e] = (i >= 0 && i < len) ? x[i] : 0.0f;
    }
    __syncthreads();
    for (int f = g0 + wave; f < g_end; f += NT_E / 64) {            // uniform over the wave
        if (f >= n_fr) {
            if (lane == 0) out[f] = 0.0f;
            continue;
        }
        const float* a = xs + (f - g0) * hop;
        float v = 0.0f;
        for (int j = lane; j < W; j += 64) v = fmaf(a[j], a[j], v);
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        if (lane == 0) out[f] = v;
    }
}

// Inclusive scans over the 1,024 lanes' values in LDS: sa by max from the left, sb by min from the right.
__device__ inline void scan_max_min(int* sa, int* sb) {
    const int t = threadIdx.x;
    for (int s = 1; s < NT_U; s <<= 1) {
        const int x = t >= s ? sa[t - s] : -1;
        const int y = t + s < NT_U ? sb[t + s] : 0x7fffffff;
        __syncthreads();
        sa[t] = max(sa[t], x);
        sb[t] = min(sb[t], y);
        __syncthreads();
    }
}

// Inclusive sum scans of sa and sb from the left.
__device__ inline void scan_sum2(int* sa, int* sb) {
    const int t = threadIdx.x;
    for (int s = 1; s < NT_U; s <<= 1) {
        const int x = t >= s ? sa[t - s] : 0;
        const int y = t >= s ? sb[t - s] : 0;
        __syncthreads();
        sa[t] += x;
        sb[t] += y;
        __syncthreads();
    }
}

// One smoothing pass over m[0 .. F).  A frame whose value is not v lies in a run bounded by the previous frame p of value
// v (-1: none) and the next one n (F: none); the run is n - p - 1 frames long.  fill: the frame takes the value v when both
// bounds exist and the run is at most `limit` long (gaps between active frames).  Otherwise: it takes v when the run is
// shorter than `limit`, bounds or not (short active runs, those at either end counted with their own length).
__device__ inline void smooth_pass(uint8_t* m, int F, int C, int v, int limit, bool fill, int* sa, int* sb) {
    const int t = threadIdx.x;
    const int c0 = min(t * C, F), c1 = min(c0 + C, F);
    int last = -1, first = 0x7fffffff;
    for (int f = c0; f < c1; ++f)
        if (m[f] == v) { last = f; if (first == 0x7fffffff) first = f; }
    sa[t] = last;
    sb[t] = first;
    __syncthreads();
    scan_max_min(sa, sb);
    int p = t > 0 ? sa[t - 1] : -1;
    const int n_after = t + 1 < NT_U ? min(sb[t + 1], F) : F;
    unsigned flip = 0;                                              // C <= 16 frames per lane
    for (int f = c0; f < c1; ++f) {
        if (m[f] == v) { p = f; continue; }
        int n = n_after;
        for (int g = f + 1; g < c1; ++g)
            if (m[g] == v) { n = g; break; }
        const int run = n - p - 1;
        const bool take = fill ? (p >= 0 && n < F && run <= limit) : (run < limit);
        if (take) flip |= 1u << (f - c0);
    }
    __syncthreads();                                                // every lane has read its neighbours' frames
    for (int f = c0; f < c1; ++f)
        if (flip & (1u << (f - c0))) m[f] = (uint8_t)v;
    __syncthreads();
}

__global__ void __launch_bounds__(NT_U)
activity_mask_kernel(const float* __restrict__ energy, const float* __restrict__ f0, const int32_t* __restrict__ n_frames,
                     int max_frames, int mode, float ratio, int max_gap, int min_run, uint8_t* __restrict__ mask) {
    __shared__ uint8_t m[MAX_FRAMES];
    __shared__ int sa[NT_U], sb[NT_U];
    __shared__ float red[NT_U / 64];
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    const int F = min(max(n_frames[b], 1), max_frames);
    const int C = (F + NT_U - 1) / NT_U;
    const float* __restrict__ E = energy + (size_t)b * max_frames;
    const float* __restrict__ P = f0 ? f0 + (size_t)b * max_frames : nullptr;
    float thr = 0.0f;
    if (mode & 1) {
        float mx = 0.0f;                                            // energies are sums of squares: none is below zero
        for (int f = t; f < F; f += NT_U) mx = fmaxf(mx, E[f]);
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
        if ((t & 63) == 0) red[t >> 6] = mx;
        __syncthreads();
        mx = red[0];
        for (int w = 1; w < NT_U / 64; ++w) mx = fmaxf(mx, red[w]);
        thr = ratio * mx;
    }
    for (int f = t; f < F; f += NT_U) {
        bool a = true;
        if (mode & 1) { const float e = E[f]; a = e > 0.0f && e > thr; }
        if (mode & 2) a = a && P[f] > 0.0f;
        m[f] = a ? 1 : 0;
    }
    __syncthreads();
    if (max_gap > 0) smooth_pass(m, F, C, 1, max_gap, true, sa, sb);
    if (min_run > 1) smooth_pass(m, F, C, 0, min_run, false, sa, sb);
    uint8_t* out = mask + (size_t)b * max_frames;
    for (int f = t; f < max_frames; f += NT_U) out[f] = f < F ? m[f] : (uint8_t)0;
}

__global__ void __launch_bounds__(NT_U)
mask_compact_kernel(const uint8_t* __restrict__ mask_a, const int32_t* __restrict__ frames_a, int max_a,
                    const uint8_t* __restrict__ mask_b, const int32_t* __restrict__ frames_b, int max_b, int32_t* __restrict__ index,
                    int32_t* __restrict__ n_active, int32_t* __restrict__ n_kept, int32_t* __restrict__ intervals,
                    int32_t* __restrict__ n_intervals) {
    __shared__ uint8_t m[MAX_FRAMES];
    __shared__ int sa[NT_U], sb[NT_U];
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    int F = min(max(frames_a[b], 1), max_a);
    if (mask_b) F = min(F, min(max(frames_b[b], 1), max_b));
    const int C = (F + NT_U - 1) / NT_U;
    const uint8_t* __restrict__ A = mask_a + (size_t)b * max_a;
    const uint8_t* __restrict__ B = mask_b ? mask_b + (size_t)b * max_b : nullptr;
    for (int f = t; f < F; f += NT_U) m[f] = (A[f] != 0 && (!B || B[f] != 0)) ? 1 : 0;
    __syncthreads();
    const int c0 = min(t * C, F), c1 = min(c0 + C, F);
    int cnt = 0, starts = 0;
    for (int f = c0; f < c1; ++f)
        if (m[f]) { ++cnt; if (f == 0 || !m[f - 1]) ++starts; }
    sa[t] = cnt;
    sb[t] = starts;
    __syncthreads();
    scan_sum2(sa, sb);
    const int total = sa[NT_U - 1], n_int = sb[NT_U - 1];
    const int max_int = (max_a + 1) / 2;
    int32_t* idx = index + (size_t)b * max_a;
    int32_t* iv = intervals + (size_t)b * max_int * 2;
    int k = sa[t] - cnt, s = sb[t] - starts;                        // the exclusive sums
    for (int f = c0; f < c1; ++f) {
        if (!m[f]) continue;
        idx[k++] = f;
        if (f == 0 || !m[f - 1]) iv[2 * s++] = f;
        if (f == F - 1 || !m[f + 1]) iv[2 * (s - 1) + 1] = f + 1;
    }
    const int kept = total > 0 ? total : F;                         // no active frame: the utterance keeps all its frames
    if (total == 0)
        for (int f = t; f < F; f += NT_U) idx[f] = f;
    for (int f = kept + t; f < max_a; f += NT_U) idx[f] = -1;
    for (int e = 2 * n_int + t; e < 2 * max_int; e += NT_U) iv[e] = -1;
    if (t == 0) { n_active[b] = total; n_kept[b] = kept; n_intervals[b] = n_int; }
}

__global__ void __launch_bounds__(NT_G)
compact_rows_kernel(const float* __restrict__ src, int src_frames, const int32_t* __restrict__ index, int index_frames,
                    const int32_t* __restrict__ n_kept, int n_cols, float* __restrict__ dst, int dst_frames) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * NT_G + threadIdx.x;
    if (e >= dst_frames * n_cols) return;
    const int k = e / n_cols, c = e - k * n_cols;
    const int kept = min(max(n_kept[b], 0), index_frames);
    float v = 0.0f;
    if (k < kept) {
        const int f = index[(size_t)b * index_frames + k];
        if (f >= 0 && f < src_frames) v = src[((size_t)b * src_frames + f) * n_cols + c];
    }
    dst[(size_t)b * dst_frames * n_cols + e] = v;
}

// path_in NULL: the cells (p, p)
__global__ void __launch_bounds__(NT_G)
path_map_kernel(const int32_t* __restrict__ path_in, const int32_t* __restrict__ path_len, int max_path,
                const int32_t* __restrict__ index_a, int max_a, const int32_t* __restrict__ index_b, int max_b,
                int32_t* __restrict__ path_out) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * NT_G + threadIdx.x;
    if (p >= max_path) return;
    const int n = min(max(path_len[b], 0), max_path);
    const size_t o = ((size_t)b * max_path + p) * 2;
    int i = -1, j = -1;
    if (p < n) {
        i = path_in ? path_in[o] : p;
        j = path_in ? path_in[o + 1] : p;
        if (i >= 0 && i < max_a && j >= 0 && j < max_b) {
            i = index_a[(size_t)b * max_a + i];
            j = index_b[(size_t)b * max_b + j];
        } else {
            i = j = -1;
        }
    }
    path_out[o] = i;
    path_out[o + 1] = j;
}

// gain[b] = target * n / sum |x[i]| over the samples of the active frames' hops (sample i belongs to frame
// min((i + hop / 2) / hop, F - 1)); over all samples when no frame is active; 1 when those are all zero.  Lane t adds
// samples t, t + 1024, ... in float64, the 1,024 partial sums are added in a fixed tree.
__global__ void __launch_bounds__(NT_U)
speech_gain_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, int max_len, int ld, int hop,
                   const uint8_t* __restrict__ mask, const int32_t* __restrict__ n_active, int max_frames, float target,
                   float* __restrict__ gain) {
    __shared__ double ss[NT_U];
    __shared__ double sn[NT_U];
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    const int F = min(1 + len / hop, max_frames);
    const bool all = n_active[b] <= 0;
    const float* __restrict__ x = wav + (size_t)b * ld;
    const uint8_t* __restrict__ m = mask + (size_t)b * max_frames;
    double s = 0.0, n = 0.0;
    for (int i = t; i < len; i += NT_U) {
        const int f = min((i + hop / 2) / hop, F - 1);
        if (all || m[f]) { s += (double)fabsf(x[i]); n += 1.0; }
    }
    ss[t] = s;
    sn[t] = n;
    __syncthreads();
    for (int w = NT_U / 2; w > 0; w >>= 1) {
        if (t < w) { ss[t] += ss[t + w]; sn[t] += sn[t + w]; }
        __syncthreads();
    }
    if (t == 0) gain[b] = ss[0] > 0.0 ? (float)((double)target * sn[0] / ss[0]) : 1.0f;
}

__global__ void __launch_bounds__(NT_G)
scale_rows_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, int max_len, int ld,
                  const float* __restrict__ gain, float* __restrict__ out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * NT_G + threadIdx.x;
    if (i >= max_len) return;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    out[(size_t)b * max_len + i] = i < len ? gain[b] * wav[(size_t)b * ld + i] : 0.0f;
}

}  // namespace

extern "C" {

int vc_frame_energy_tile(int32_t hop, int32_t frame_length) {
    if (hop < 1 || frame_length < 1 || hop > MAX_HOP || frame_length > MAX_W) return 0;
    return energy_tile(frame_length, hop);
}

int vc_frame_energy_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, int32_t hop,
                        int32_t frame_length, float* d_energy, int32_t max_frames, void* stream) {
    VC_REQUIRE(d_wav && d_energy, "vc_frame_energy_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1 && ld >= max_len && hop >= 1 && frame_length >= 1,
               "vc_frame_energy_f32: bad shape (batch %d, max_len %d, ld %d, hop %d, frame_length %d; need all >= 1 and ld >= max_len)",
               batch, max_len, ld, hop, frame_length);
    VC_REQUIRE(max_frames >= 1, "vc_frame_energy_f32: max_frames must be at least 1 (got %d)", max_frames);
    if (batch > 65535 || max_len > MAX_SAMPLES || frame_length > MAX_W || hop > MAX_HOP || max_frames > MAX_SAMPLES + 1)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_frame_energy_f32: limits are batch <= 65535, max_len <= %d, frame_length <= %d, "
                             "hop <= %d, max_frames <= %d; got batch %d, max_len %d, frame_length %d, hop %d, max_frames %d", MAX_SAMPLES,
                             MAX_W, MAX_HOP, MAX_SAMPLES + 1, batch, max_len, frame_length, hop, max_frames);
    VC_REQUIRE(max_frames >= 1 + max_len / hop, "vc_frame_energy_f32: max_frames %d is less than 1 + max_len / hop = %d", max_frames,
               1 + max_len / hop);
    const int G = energy_tile(frame_length, hop);
    const dim3 grid((unsigned)((max_frames + G - 1) / G), (unsigned)batch);
    hipLaunchKernelGGL(frame_energy_kernel, grid, dim3(NT_E), energy_lds_bytes(frame_length, hop, G), static_cast<hipStream_t>(stream),
                       d_wav, d_lens, max_len, ld, hop, frame_length, G, d_energy, max_frames);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_activity_mask(const float* d_energy, const float* d_f0, const int32_t* d_n_frames, int32_t batch, int32_t max_frames,
                     int32_t mode, float ratio, int32_t max_gap, int32_t min_run, uint8_t* d_mask, void* stream) {
    VC_REQUIRE(d_n_frames && d_mask, "vc_activity_mask: NULL argument");
    VC_REQUIRE(mode >= 1 && mode <= 3, "vc_activity_mask: mode must be 1 (energy), 2 (voiced) or 3 (both), got %d", mode);
    VC_REQUIRE(!(mode & 1) || d_energy, "vc_activity_mask: the energy modes need d_energy");
    VC_REQUIRE(!(mode & 2) || d_f0, "vc_activity_mask: the voiced modes need d_f0");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && max_gap >= 0 && min_run >= 0,
               "vc_activity_mask: bad shape (batch %d, max_frames %d, max_gap %d, min_run %d)", batch, max_frames, max_gap, min_run);
    VC_REQUIRE(!(mode & 1) || (std::isfinite(ratio) && ratio > 0.0f && ratio < 1.0f),
               "vc_activity_mask: the ratio 10^(-top_db / 10) must lie in (0, 1), got %g", (double)ratio);
    if (batch > 65535 || max_frames > MAX_FRAMES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_activity_mask: limits are batch <= 65535 and max_frames <= %d; got batch %d, "
                             "max_frames %d", MAX_FRAMES, batch, max_frames);
    hipLaunchKernelGGL(activity_mask_kernel, dim3(batch), dim3(NT_U), 0, static_cast<hipStream_t>(stream), d_energy, d_f0, d_n_frames,
                       max_frames, mode, ratio, max_gap, min_run, d_mask);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_mask_compact(const uint8_t* d_mask_a, const int32_t* d_frames_a, int32_t max_a, const uint8_t* d_mask_b,
                    const int32_t* d_frames_b, int32_t max_b, int32_t batch, int32_t* d_index, int32_t* d_n_active, int32_t* d_n_kept,
                    int32_t* d_intervals, int32_t* d_n_intervals, void* stream) {
    VC_REQUIRE(d_mask_a && d_frames_a && d_index && d_n_active && d_n_kept && d_intervals && d_n_intervals,
               "vc_mask_compact: NULL argument");
    VC_REQUIRE((d_mask_b == nullptr) == (d_frames_b == nullptr) && (d_mask_b ? max_b >= 1 : max_b == 0),
               "vc_mask_compact: pass d_mask_b, d_frames_b and max_b >= 1 together, or NULL, NULL and 0 (max_b %d)", max_b);
    VC_REQUIRE(batch >= 1 && max_a >= 1, "vc_mask_compact: bad shape (batch %d, max_a %d)", batch, max_a);
    if (batch > 65535 || max_a > MAX_FRAMES || max_b > MAX_FRAMES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_mask_compact: limits are batch <= 65535 and max_a, max_b <= %d; got batch %d, max_a "
                             "%d, max_b %d", MAX_FRAMES, batch, max_a, max_b);
    hipLaunchKernelGGL(mask_compact_kernel, dim3(batch), dim3(NT_U), 0, static_cast<hipStream_t>(stream), d_mask_a, d_frames_a, max_a,
                       d_mask_b, d_frames_b, max_b, d_index, d_n_active, d_n_kept, d_intervals, d_n_intervals);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_compact_rows_f32(const float* d_src, int32_t src_frames, const int32_t* d_index, int32_t index_frames, const int32_t* d_n_kept,
                        int32_t batch, int32_t n_cols, float* d_dst, int32_t dst_frames, void* stream) {
    VC_REQUIRE(d_src && d_index && d_n_kept && d_dst, "vc_compact_rows_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && src_frames >= 1 && index_frames >= 1 && dst_frames >= 1 && n_cols >= 1,
               "vc_compact_rows_f32: bad shape (batch %d, src_frames %d, index_frames %d, dst_frames %d, n_cols %d)", batch, src_frames,
               index_frames, dst_frames, n_cols);
    if (batch > 65535 || src_frames > MAX_FRAMES || index_frames > MAX_FRAMES || dst_frames > MAX_FRAMES || n_cols > MAX_COLS)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_compact_rows_f32: limits are batch <= 65535, frames <= %d, n_cols <= %d; got batch "
                             "%d, src_frames %d, index_frames %d, dst_frames %d, n_cols %d", MAX_FRAMES, MAX_COLS, batch, src_frames,
                             index_frames, dst_frames, n_cols);
    const dim3 grid((unsigned)((dst_frames * n_cols + NT_G - 1) / NT_G), (unsigned)batch);
    hipLaunchKernelGGL(compact_rows_kernel, grid, dim3(NT_G), 0, static_cast<hipStream_t>(stream), d_src, src_frames, d_index,
                       index_frames, d_n_kept, n_cols, d_dst, dst_frames);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_path_map(const int32_t* d_path_in, const int32_t* d_path_len, int32_t batch, int32_t max_path, const int32_t* d_index_a,
                int32_t max_a, const int32_t* d_index_b, int32_t max_b, int32_t* d_path_out, void* stream) {
    VC_REQUIRE(d_path_len && d_index_a && d_index_b && d_path_out, "vc_path_map: NULL argument");
    VC_REQUIRE(batch >= 1 && max_path >= 1 && max_a >= 1 && max_b >= 1, "vc_path_map: bad shape (batch %d, max_path %d, max_a %d, max_b %d)",
               batch, max_path, max_a, max_b);
    if (batch > 65535 || max_a > MAX_FRAMES || max_b > MAX_FRAMES || max_path > 2 * MAX_FRAMES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_path_map: limits are batch <= 65535, max_a, max_b <= %d, max_path <= %d; got batch %d, "
                             "max_a %d, max_b %d, max_path %d", MAX_FRAMES, 2 * MAX_FRAMES, batch, max_a, max_b, max_path);
    const dim3 grid((unsigned)((max_path + NT_G - 1) / NT_G), (unsigned)batch);
    hipLaunchKernelGGL(path_map_kernel, grid, dim3(NT_G), 0, static_cast<hipStream_t>(stream), d_path_in, d_path_len, max_path,
                       d_index_a, max_a, d_index_b, max_b, d_path_out);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_speech_gain_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, int32_t hop,
                       const uint8_t* d_mask, const int32_t* d_n_active, int32_t max_frames, float target, float* d_gain,
                       void* stream) {
    VC_REQUIRE(d_wav && d_mask && d_n_active && d_gain, "vc_speech_gain_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1 && ld >= max_len && hop >= 1 && max_frames >= 1,
               "vc_speech_gain_f32: bad shape (batch %d, max_len %d, ld %d, hop %d, max_frames %d)", batch, max_len, ld, hop, max_frames);
    VC_REQUIRE(std::isfinite(target) && target > 0.0f, "vc_speech_gain_f32: target must be finite and positive, got %g", (double)target);
    if (batch > 65535 || max_len > MAX_SAMPLES || hop > MAX_HOP || max_frames > MAX_FRAMES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_speech_gain_f32: limits are batch <= 65535, max_len <= %d, hop <= %d, max_frames <= %d; "
                             "got batch %d, max_len %d, hop %d, max_frames %d", MAX_SAMPLES, MAX_HOP, MAX_FRAMES, batch, max_len, hop,
                             max_frames);
    VC_REQUIRE(max_frames >= 1 + max_len / hop, "vc_speech_gain_f32: max_frames %d is less than 1 + max_len / hop = %d", max_frames,
               1 + max_len / hop);
    hipLaunchKernelGGL(speech_gain_kernel, dim3(batch), dim3(NT_U), 0, static_cast<hipStream_t>(stream), d_wav, d_lens, max_len, ld, hop,
                       d_mask, d_n_active, max_frames, target, d_gain);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_scale_rows_f32(const float* d_wav, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, const float* d_gain,
                      float* d_out, void* stream) {
    VC_REQUIRE(d_wav && d_gain && d_out, "vc_scale_rows_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_len >= 1 && ld >= max_len, "vc_scale_rows_f32: bad shape (batch %d, max_len %d, ld %d)", batch, max_len, ld);
    if (batch > 65535 || max_len > MAX_SAMPLES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_scale_rows_f32: limits are batch <= 65535 and max_len <= %d; got batch %d, max_len %d",
                             MAX_SAMPLES, batch, max_len);
    const dim3 grid((unsigned)((max_len + NT_G - 1) / NT_G), (unsigned)batch);
    hipLaunchKernelGGL(scale_rows_kernel, grid, dim3(NT_G), 0, static_cast<hipStream_t>(stream), d_wav, d_lens, max_len, ld, d_gain, d_out);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
