// Postfilters for converted spectra (include/vc_hip.h, "Postfilters"): the global-variance filter (Toda) and the
// modulation-spectrum filter (Takamichi) on trajectories x [B, maxF, C] float32, C contiguous.  One lane per channel in
// every kernel, so a wave reads and writes rows of 64 channels coalesced and nothing is transposed; a lane walks time.
//
//   traj_stats_kernel  grid (channel tiles of 64, B), 8 waves: wave w sums the frames f = w, w + 8, ... of its channels in
//                      ascending f, the eight partial sums meet in LDS and are added in ascending w.  Two passes over the
//                      utterance: the mean about the first frame, then the squared deviations from the mean.
//   gv_filter_kernel   grid (tiles of 32 frames, channel tiles, B), 4 waves of 8 frames each: y = x + (g - 1)(x - mean).
//   ms_stats_kernel    grid (channel tiles, B), 4 waves: wave w takes the segments j = w, w + 4, ... in ascending j, a 64-point
//                      real transform per lane in registers; count, sum s and sum s^2 of the 33 bins stay in registers and
//                      meet in LDS in three rounds (one per quantity), added in ascending w.
//   ms_filter_kernel   grid (tiles of 32 frames, channel tiles, B), 1 wave: the workgroup owns 32 output frames and computes
//                      both segments that cover them (forward transform, gain, inverse transform of (g - 1) X, of which only
//                      the half that falls on the tile is formed), adds the two corrections and writes every element once.
//                      The tile's coefficients go through LDS: read straight from the [C, 33, 2] table a lane's 66 values lie
//                      264 bytes from its neighbour's, 64 cache lines per load instruction.
//
// The 64-point real transform: z[k] = v[2k] + i v[2k+1], a 32-point complex transform as two of fe_dft400.h's 16-point ones
// (even and odd k) joined by W32^k, then the usual untangling into bins 0 .. 32.  The inverse runs the same steps backwards.
// Everything is unrolled, twiddles and window are constants, and every array index is known at compile time: the arrays are
// registers.  No atomics, no allocation, no host wait; n_frames is clamped to [0, maxF] when read and a frame index outside
// [0, n) is never an address (edge hold clamps it into the utterance).
#include <cmath>
#include "vc_common.h"
#include "pf_dft64.h"

namespace {

using namespace vcpf;

constexpr int PF_MAX_BATCH = 65535, PF_MAX_FRAMES = 16384, PF_MAX_CHANNELS = 2049;
constexpr int SEG = 64, HOP = 32, NBIN = 33;
constexpr int ST_NW = 8;                // waves of traj_stats_kernel
constexpr int MS_NW = 4;                // waves of ms_stats_kernel
constexpr int GV_NW = 4;                // waves of gv_filter_kernel
constexpr int COEF_LD = 2 * NBIN + 1;   // a channel's 66 coefficients in LDS: an odd stride, so 64 lanes hit 32 banks twice and no more
constexpr float VAR_TINY = 9.094947017729282e-13f;      // 2^-40: at or below it a channel counts as constant
constexpr float MS_FLOOR = 1.0e-20f;    // |X|^2 at or below it: the bin is not counted and its gain is 1
constexpr float F32_MAX = 3.402823466e38f;

__device__ __forceinline__ int clamp_frames(const int32_t* n_frames, int b, int maxF) {
    return n_frames ? min(max(n_frames[b], 0), maxF) : maxF;
}

// v[t] = w[t] (x[hold(32 j - 32 + t)] - mean): segment j of one channel, frames outside [0, n) held at the edge (n >= 1)
__device__ __forceinline__ void load_segment(const float* __restrict__ xc, size_t C, int n, int j, float mean, float* v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int t = 0; t < SEG; ++t) {
        const int f = min(max(HOP * j - HOP + t, 0), n - 1);
        v[t] = WIN[t] * (xc[(size_t)f * C] - mean);
    }
}

// ------------------------------------------------------------------------------------------ statistics of a trajectory
__global__ void __launch_bounds__(ST_NW * 64)
traj_stats_kernel(const float* __restrict__ x, const int32_t* __restrict__ n_frames, int maxF, int C, float* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ float part[ST_NW][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
    const int c = blockIdx.x * 64 + lane, cc = min(c, C - 1);
    const int n = clamp_frames(n_frames, b, maxF);
    const float* xc = x + (size_t)b * maxF * C + cc;
    const float ref = n > 0 ? xc[0] : 0.0f;
    float acc = 0.0f;
#pragma unroll 4
    for (int f = w; f < n; f += ST_NW) acc += xc[(size_t)f * C] - ref;
    part[w][lane] = acc;
    __syncthreads();
    float tot = part[0][lane];
#pragma unroll
    for (int k = 1; k < ST_NW; ++k) tot += part[k][lane];
    const float mean = n > 0 ? ref + tot / (float)n : 0.0f;
    __syncthreads();                                                // every wave has read the partial sums
    acc = 0.0f;
#pragma unroll 4
    for (int f = w; f < n; f += ST_NW) {
        const float d = xc[(size_t)f * C] - mean;
        acc += d * d;
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && c < C) {
        tot = part[0][lane];
#pragma unroll
        for (int k = 1; k < ST_NW; ++k) tot += part[k][lane];
        float* o = stats + ((size_t)b * C + c) * 2;
        o[0] = mean;
        o[1] = n > 0 ? tot / (float)n : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------ global-variance filter
__global__ void __launch_bounds__(GV_NW * 64)
gv_filter_kernel(const float* __restrict__ x, const int32_t* __restrict__ n_frames, const float* __restrict__ stats,
                 const float* __restrict__ gv_t, int maxF, int C, float alpha, float g_max, float* __restrict__ y) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.z;
    const int c = blockIdx.y * 64 + lane;
    if (c >= C) return;
    const int n = clamp_frames(n_frames, b, maxF);
    const int f0 = blockIdx.x * HOP + w * (HOP / GV_NW);
    const float mean = stats[((size_t)b * C + c) * 2], var = stats[((size_t)b * C + c) * 2 + 1], target = gv_t[c];
    float gm1 = 0.0f;
    if (var > VAR_TINY && target > 0.0f) {
        const float q = target / var;
        if (q <= F32_MAX) {
            const float r = sqrtf(q) - 1.0f;
            const float g = 1.0f + alpha * r;
            gm1 = fminf(fmaxf(g, 1.0f / g_max), g_max) - 1.0f;
        }
    }
    const size_t base = (size_t)b * maxF * C + c;
#pragma unroll
    for (int i = 0; i < HOP / GV_NW; ++i) {
        const int f = f0 + i;
        if (f >= maxF) break;
        float out = 0.0f;
        if (f < n) {
            const float xv = x[base + (size_t)f * C];
            const float d = gm1 * (xv - mean);
            out = d == 0.0f ? xv : xv + d;
        }
        y[base + (size_t)f * C] = out;
    }
}

// ------------------------------------------------------------------------------------------ modulation-spectrum statistics
__global__ void __launch_bounds__(MS_NW * 64)
ms_stats_kernel(const float* __restrict__ x, const int32_t* __restrict__ n_frames, const float* __restrict__ stats, int maxF,
                int C, float* __restrict__ ms) {
#pragma clang fp contract(off)
    __shared__ float part[MS_NW][NBIN][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
    const int c = blockIdx.x * 64 + lane, cc = min(c, C - 1);
    const int n = clamp_frames(n_frames, b, maxF);
    const float* xc = x + (size_t)b * maxF * C + cc;
    const float mean = stats[((size_t)b * C + cc) * 2];
    float cnt[NBIN], sm[NBIN], sq[NBIN];
#pragma unroll
    for (int m = 0; m < NBIN; ++m) { cnt[m] = 0.0f; sm[m] = 0.0f; sq[m] = 0.0f; }
    const int J = n > 0 ? (n + HOP - 1) / HOP : -1;                 // segments 0 .. J
    for (int j = w; j <= J; j += MS_NW) {
        float v[SEG], xr[NBIN], xi[NBIN];
        load_segment(xc, (size_t)C, n, j, mean, v);
        rdft64(v, xr, xi);
#pragma unroll
        for (int m = 0; m < NBIN; ++m) {
            const float p = xr[m] * xr[m] + xi[m] * xi[m];
            if (p > MS_FLOOR && p <= F32_MAX) {
                const float s = logf(p);
                cnt[m] += 1.0f;
                sm[m] += s;
                sq[m] += s * s;
            }
        }
    }
    float* o = ms + ((size_t)b * C + cc) * (NBIN * 3);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int m = 0; m < NBIN; ++m) part[w][m][lane] = r == 0 ? cnt[m] : r == 1 ? sm[m] : sq[m];
        __syncthreads();
        if (w == 0 && c < C) {
#pragma unroll
            for (int m = 0; m < NBIN; ++m) {
                float tot = part[0][m][lane];
#pragma unroll
                for (int k = 1; k < MS_NW; ++k) tot += part[k][m][lane];
                o[m * 3 + r] = tot;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ modulation-spectrum filter
// The correction of segment j on its samples [32 * HALF, 32 * HALF + 32): iDFT64((g - 1) X_j).
template <int HALF>
__device__ __forceinline__ void ms_correction(const float* __restrict__ xc, size_t C, int n, int j, float mean,
                                              const float* coef_c, float lo, float hi, float* out) {
#pragma clang fp contract(off)
    float v[SEG], xr[NBIN], xi[NBIN];
    load_segment(xc, C, n, j, mean, v);
    rdft64(v, xr, xi);
    xr[0] = 0.0f; xi[0] = 0.0f;                                     // g_0 = 1
#pragma unroll
    for (int m = 1; m < NBIN; ++m) {
        const float p = xr[m] * xr[m] + xi[m] * xi[m];
        float gm1 = 0.0f;
        if (p > MS_FLOOR && p <= F32_MAX) {
            const float e = coef_c[2 * m] * logf(p) + coef_c[2 * m + 1];
            gm1 = expf(fminf(fmaxf(e, lo), hi)) - 1.0f;
        }
        xr[m] *= gm1; xi[m] *= gm1;
    }
    irdft64_half<HALF>(xr, xi, out);
}

__global__ void __launch_bounds__(64)
ms_filter_kernel(const float* __restrict__ x, const int32_t* __restrict__ n_frames, const float* __restrict__ stats,
                 const float* __restrict__ coef, int maxF, int C, float lo, float hi, float* __restrict__ y) {
#pragma clang fp contract(off)
    __shared__ float coef_l[64 * COEF_LD];
    const int t = blockIdx.x, b = blockIdx.z;
    const int c0 = blockIdx.y * 64, lane = (int)threadIdx.x, c = c0 + lane;
    const int n = clamp_frames(n_frames, b, maxF);
    const int f0 = t * HOP;
    if (f0 < n) {                                                   // (uniform) the tile's 64 x 66 coefficients are one contiguous
        const int cnt = min(64, C - c0) * (NBIN * 2);               //  stretch: read coalesced, kept in LDS at an odd row stride
        const float* src = coef + (size_t)c0 * (NBIN * 2);
#pragma unroll 6
        for (int i = lane; i < cnt; i += 64) coef_l[(i / (NBIN * 2)) * COEF_LD + i % (NBIN * 2)] = src[i];
        __syncthreads();
    }
    if (c >= C) return;
    const size_t base = (size_t)b * maxF * C + c;
    if (f0 >= n) {                                                  // (uniform) a tile beyond the utterance: zeros
#pragma unroll 4
        for (int i = 0; i < HOP; ++i)
            if (f0 + i < maxF) y[base + (size_t)(f0 + i) * C] = 0.0f;
        return;
    }
    const float mean = stats[((size_t)b * C + c) * 2];
    const float* coef_c = coef_l + lane * COEF_LD;
    float ca[HOP], cb[HOP];
    ms_correction<1>(x + base, (size_t)C, n, t, mean, coef_c, lo, hi, ca);          // segment t: the tile is its later half
    ms_correction<0>(x + base, (size_t)C, n, t + 1, mean, coef_c, lo, hi, cb);      // segment t + 1: its earlier half
#pragma unroll
    for (int i = 0; i < HOP; ++i) {
        const int f = f0 + i;
        if (f < maxF) {
            float out = 0.0f;
            if (f < n) {
                const float xv = x[base + (size_t)f * C];
                const float d = ca[i] + cb[i];
                out = d == 0.0f ? xv : xv + d;
            }
            y[base + (size_t)f * C] = out;
        }
    }
}

// VC_OK, or the refusal's code with the message set
int pf_check(const char* who, const void* a, const void* b, const void* c, const void* d, int batch, int max_frames, int channels) {
    VC_REQUIRE(a && b && c && d, "%s: NULL argument", who);
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && channels >= 1, "%s: bad shape (batch %d, max_frames %d, channels %d)", who, batch,
               max_frames, channels);
    if (batch > PF_MAX_BATCH || max_frames > PF_MAX_FRAMES || channels > PF_MAX_CHANNELS)
        return vc::set_error(VC_ERR_UNSUPPORTED, "%s: limits are batch <= %d, max_frames <= %d, channels <= %d; got %d, %d, %d", who,
                             PF_MAX_BATCH, PF_MAX_FRAMES, PF_MAX_CHANNELS, batch, max_frames, channels);
    return VC_OK;
}

inline bool finite_f(float v) { return v == v && v >= -F32_MAX && v <= F32_MAX; }

}  // namespace

extern "C" {

int vc_traj_stats_f32(const float* d_x, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t channels,
                      float* d_stats, void* stream) {
    const int rc = pf_check("vc_traj_stats_f32", d_x, d_stats, d_x, d_x, batch, max_frames, channels);
    if (rc != VC_OK) return rc;
    hipLaunchKernelGGL(traj_stats_kernel, dim3((channels + 63) / 64, batch), dim3(ST_NW * 64), 0, static_cast<hipStream_t>(stream),
                       d_x, d_n_frames, max_frames, channels, d_stats);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_gv_filter_f32(const float* d_x, const int32_t* d_n_frames, const float* d_stats, const float* d_gv_t, int32_t batch,
                     int32_t max_frames, int32_t channels, float alpha, float g_max, float* d_y, void* stream) {
    VC_REQUIRE(finite_f(alpha) && alpha >= 0.0f && alpha <= 1.0f, "vc_gv_filter_f32: alpha must lie in [0, 1]");
    VC_REQUIRE(finite_f(g_max) && g_max >= 1.0f, "vc_gv_filter_f32: g_max must be finite and at least 1");
    const int rc = pf_check("vc_gv_filter_f32", d_x, d_stats, d_gv_t, d_y, batch, max_frames, channels);
    if (rc != VC_OK) return rc;
    VC_REQUIRE(d_y != d_x, "vc_gv_filter_f32: d_y must not be d_x");
    hipLaunchKernelGGL(gv_filter_kernel, dim3((max_frames + HOP - 1) / HOP, (channels + 63) / 64, batch), dim3(GV_NW * 64), 0,
                       static_cast<hipStream_t>(stream), d_x, d_n_frames, d_stats, d_gv_t, max_frames, channels, alpha, g_max, d_y);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_ms_stats_f32(const float* d_x, const int32_t* d_n_frames, const float* d_stats, int32_t batch, int32_t max_frames,
                    int32_t channels, float* d_ms, void* stream) {
    const int rc = pf_check("vc_ms_stats_f32", d_x, d_stats, d_ms, d_x, batch, max_frames, channels);
    if (rc != VC_OK) return rc;
    hipLaunchKernelGGL(ms_stats_kernel, dim3((channels + 63) / 64, batch), dim3(MS_NW * 64), 0, static_cast<hipStream_t>(stream), d_x,
                       d_n_frames, d_stats, max_frames, channels, d_ms);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_ms_filter_f32(const float* d_x, const int32_t* d_n_frames, const float* d_stats, const float* d_coef, int32_t batch,
                     int32_t max_frames, int32_t channels, float lo, float hi, float* d_y, void* stream) {
    VC_REQUIRE(finite_f(lo) && finite_f(hi) && lo <= 0.0f && hi >= 0.0f, "vc_ms_filter_f32: the clamps must be finite with lo <= 0 <= hi");
    const int rc = pf_check("vc_ms_filter_f32", d_x, d_stats, d_coef, d_y, batch, max_frames, channels);
    if (rc != VC_OK) return rc;
    VC_REQUIRE(d_y != d_x, "vc_ms_filter_f32: d_y must not be d_x");
    hipLaunchKernelGGL(ms_filter_kernel, dim3((max_frames + HOP - 1) / HOP, (channels + 63) / 64, batch), dim3(64), 0,
                       static_cast<hipStream_t>(stream), d_x, d_n_frames, d_stats, d_coef, max_frames, channels, lo, hi, d_y);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
