// Device-resident batched conversion (conversion.convert_batch): the three data-movement steps between the
// front-end, the decoder and the vocoder that the reference's test.py does on the host.
//
//   cut_windows_kernel      features [B, Fmax, C]      -> window batch [W, T, C]   (test.py:92-119, zero padding included)
//   compound_stitch_kernel  window batch [W, T, C]     -> utterances [B, Fout, C]  (test.py:46-84 / 134-138), optionally
//                                                         also the vocoder's magnitude (audio_lib.py:289-298, realse == 1)
//   phase_init_kernel       (seed, utt_id, frame, bin) -> initial phase [B, Fmax, bins] (audio_lib.py:255 on the device)
//
// All three stream: no LDS, no atomics, every destination element written exactly once.  A destination slab (one window,
// one utterance) is treated as a flat array whose length is a multiple of 4 floats, so every lane stores 16 aligned bytes;
// the source is read as 16 bytes (8 for bf16) when C % 4 == 0 -- a lane's four elements then lie in one row at an aligned
// address -- and element by element otherwise (C = 201, 61: a row is not a multiple of 16 bytes, so source and destination
// are not aligned alike and a lane's four elements may straddle two rows).  Slabs whose length is not a multiple of 4 take
// the same kernels with one element per lane.
#include "vc_common.h"

namespace {

constexpr int CT = 256;

__device__ __forceinline__ float load_elem(const void* src, int bf16, size_t i) {
    if (bf16) return __uint_as_float((uint32_t)static_cast<const uint16_t*>(src)[i] << 16);
    return static_cast<const float*>(src)[i];
}

// V consecutive elements of one row (C % V == 0, i % V == 0: aligned)
template <int V>
__device__ __forceinline__ void load_vec(const void* src, int bf16, size_t i, float (&v)[V]) {
    if constexpr (V == 4) {
        if (bf16) {
            const uint2 r = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(src) + i);
            v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xFFFF0000u);
            v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xFFFF0000u);
        } else {
            const float4 r = *reinterpret_cast<const float4*>(static_cast<const float*>(src) + i);
            v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
        }
    } else {
        v[0] = load_elem(src, bf16, i);
    }
}

template <int V>
__device__ __forceinline__ void store_vec(float* dst, size_t i, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[i] = v[0];
}

// ---- features -> windows.  grid (tiles of CT * V elements, W).  win_tab[w] = (utterance, first frame).
template <int V, bool ROWVEC>
__global__ void __launch_bounds__(CT)
cut_windows_kernel(const float* __restrict__ src, const int32_t* __restrict__ win_tab, const int32_t* __restrict__ n_frames,
                   int B, int Fmax, int T, int C, float* __restrict__ dst) {
    const int w = blockIdx.y;
    const int slab = T * C;
    const int i0 = (blockIdx.x * CT + threadIdx.x) * V;
    if (i0 >= slab) return;
    const int u = win_tab[2 * w], f0 = win_tab[2 * w + 1];
    int lim = 0;                                                   // elements of this window that come from the source
    if ((unsigned)u < (unsigned)B && f0 >= 0) {
        const int nf = min(max(n_frames ? n_frames[u] : Fmax, 0), Fmax);
        lim = (int)min((long long)max(nf - f0, 0) * C, (long long)slab);
    }
    const float* s = src + ((size_t)(u < 0 ? 0 : u) * Fmax + (f0 < 0 ? 0 : f0)) * C;
    float v[V];
    if (ROWVEC && i0 + V <= lim) {
        load_vec<V>(s, 0, (size_t)i0, v);                          // lim is a multiple of C, C of V: whole vector or nothing
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (i0 + k < lim) ? s[i0 + k] : 0.0f;
    }
    store_vec<V>(dst + (size_t)w * slab, (size_t)i0, v);
}

// Source row (in the [W * T] row space of the window batch) of output frame t, -1 for a zero row: the closed form of
// conversion.compound_index (test.py:58-80), the plain reshape (test.py:134-138) for one window or one pass.
__device__ __forceinline__ int stitch_row(int t, int T, int N, int w0, int w1) {
    if (t >= N * T) return -1;
    if (N == 1 || w1 < 0) return w0 * T + t;
    const int q = T / 4, h = T / 2;
    if (t < T - q) return w0 * T + t;
    if (t >= N * T - (T - q)) return (w0 + N - 1) * T + (t - (N - 1) * T);
    const int m = t - (T - q), j = m / h, r = m - j * h;
    return ((j & 1) ? w0 + (j + 1) / 2 : w1 + j / 2) * T + q + r;
}

// ---- windows -> utterances.  grid (tiles of CT * V elements, B).  utt_tab[b] = (first pass-0 window, first pass-1
// window or -1, N).  amp != NULL: also amp = exp10(0.05 * (max(0, P) * inv_norm - 80)), the expression of
// power_to_amp_kernel (vc_vocoder.hip), 0 in the zero rows.
template <int V, bool ROWVEC>
__global__ void __launch_bounds__(CT)
compound_stitch_kernel(const void* __restrict__ src, int bf16, const int32_t* __restrict__ utt_tab, int W, int T, int C,
                       int Fout, float inv_norm, float* __restrict__ dst, float* __restrict__ amp) {
    const int b = blockIdx.y;
    const int slab = Fout * C;
    const int i0 = (blockIdx.x * CT + threadIdx.x) * V;
    if (i0 >= slab) return;
    const int w0 = utt_tab[3 * b], w1 = utt_tab[3 * b + 1];
    int N = utt_tab[3 * b + 2];
    // a table that points outside the window batch yields zeros, never a stray read
    const bool two = N > 1 && w1 >= 0;
    if (N < 1 || w0 < 0 || (long long)w0 + N > W || (two && (long long)w1 + N - 1 > W) || (long long)N * T > Fout) N = 0;
    int t = i0 / C, c = i0 - t * C;
    float v[V];
    if (ROWVEC) {
        const int row = stitch_row(t, T, N, w0, w1);
        if (row >= 0) {
            load_vec<V>(src, bf16, (size_t)row * C + c, v);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = 0.0f;
        }
        if (amp) {
            float a[V];
#pragma unroll
            for (int k = 0; k < V; ++k) a[k] = row >= 0 ? vc::power_db_to_amp(v[k], inv_norm) : 0.0f;
            store_vec<V>(amp + (size_t)b * slab, (size_t)i0, a);
        }
    } else {
        float a[V];
        int row = stitch_row(t, T, N, w0, w1);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = row >= 0 ? load_elem(src, bf16, (size_t)row * C + c) : 0.0f;
            a[k] = (amp && row >= 0) ? vc::power_db_to_amp(v[k], inv_norm) : 0.0f;
            if (++c == C) { c = 0; ++t; row = stitch_row(t, T, N, w0, w1); }
        }
        if (amp) store_vec<V>(amp + (size_t)b * slab, (size_t)i0, a);
    }
    store_vec<V>(dst + (size_t)b * slab, (size_t)i0, v);
}

// ---- initial phase.  grid (tiles of CT Philox blocks, B); one block of four words = elements 4j .. 4j+3 of the
// utterance's flat [Fmax * bins] slab.  VEC: the slab length is a multiple of 4, so the four go out as one 16-byte store.
template <bool VEC>
__global__ void __launch_bounds__(CT)
phase_init_kernel(const int32_t* __restrict__ n_frames, const int32_t* __restrict__ utt_id, int Fmax, int nb,
                  uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ phase) {
    const int b = blockIdx.y;
    const long long slab = (long long)Fmax * nb;
    const long long e0 = ((long long)blockIdx.x * CT + threadIdx.x) * 4;
    if (e0 >= slab) return;
    const int nf = min(max(n_frames ? n_frames[b] : Fmax, 0), Fmax);
    const long long lim = (long long)nf * nb;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e0 < lim) {
        uint32_t x[4];
        vc::philox4x32_10((uint32_t)(e0 >> 2), (uint32_t)(utt_id ? utt_id[b] : b), 0u, 0u, seed_lo, seed_hi, x);
#pragma unroll
        for (int k = 0; k < 4; ++k)                                // one rounding: (x >> 8) * 2^-24 is exact
            v[k] = (e0 + k < lim) ? __fmul_rn(3.14159265358979323846f, (float)(x[k] >> 8) * 5.9604644775390625e-8f) : 0.0f;
    }
    float* o = phase + (size_t)b * slab;
    if (VEC) {
        *reinterpret_cast<float4*>(o + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e0 + k < slab) o[e0 + k] = v[k];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned tiles(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

extern "C" {

int vc_cut_windows(const float* d_src, const int32_t* d_win_tab, const int32_t* d_n_frames, int32_t batch,
                   int32_t max_frames, int32_t n_windows, int32_t T, int32_t C, float* d_dst, void* stream) {
    VC_REQUIRE(d_src && d_win_tab && d_dst, "vc_cut_windows: NULL argument");
    VC_REQUIRE(batch > 0 && max_frames > 0 && n_windows > 0 && n_windows <= 65535 && T > 0 && C > 0,
               "vc_cut_windows: bad shape (batch %d, max_frames %d, n_windows %d, T %d, C %d)", batch, max_frames, n_windows, T, C);
    VC_REQUIRE((long long)T * C < (1ll << 30) && (long long)batch * max_frames * C < (1ll << 40), "vc_cut_windows: too large");
    const long long slab = (long long)T * C;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (slab % 4) == 0 && aligned16(d_dst);
    if (vec && (C % 4) == 0 && aligned16(d_src))
        hipLaunchKernelGGL((cut_windows_kernel<4, true>), dim3(tiles(slab, CT * 4), n_windows), dim3(CT), 0, st, d_src, d_win_tab,
                           d_n_frames, batch, max_frames, T, C, d_dst);
    else if (vec)
        hipLaunchKernelGGL((cut_windows_kernel<4, false>), dim3(tiles(slab, CT * 4), n_windows), dim3(CT), 0, st, d_src, d_win_tab,
                           d_n_frames, batch, max_frames, T, C, d_dst);
    else
        hipLaunchKernelGGL((cut_windows_kernel<1, false>), dim3(tiles(slab, CT), n_windows), dim3(CT), 0, st, d_src, d_win_tab,
                           d_n_frames, batch, max_frames, T, C, d_dst);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_compound_stitch(const void* d_src, int32_t src_dtype, const int32_t* d_utt_tab, int32_t batch, int32_t n_windows,
                       int32_t T, int32_t C, int32_t out_frames, float* d_dst, float* d_amp, float P_dB_norm_factor,
                       void* stream) {
    VC_REQUIRE(d_src && d_utt_tab && d_dst, "vc_compound_stitch: NULL argument");
    VC_REQUIRE(src_dtype == VC_F32 || src_dtype == VC_BF16, "vc_compound_stitch: src_dtype must be VC_F32 or VC_BF16");
    VC_REQUIRE(batch > 0 && batch <= 65535 && n_windows > 0 && T > 0 && (T % 4) == 0 && C > 0 && out_frames > 0,
               "vc_compound_stitch: bad shape (batch %d, n_windows %d, T %d (multiple of 4), C %d, out_frames %d)", batch,
               n_windows, T, C, out_frames);
    VC_REQUIRE((long long)out_frames * C < (1ll << 30) && (long long)n_windows * T * C < (1ll << 40), "vc_compound_stitch: too large");
    VC_REQUIRE(!d_amp || src_dtype == VC_F32, "vc_compound_stitch: the magnitude flavour takes a float32 source");
    VC_REQUIRE(!d_amp || P_dB_norm_factor != 0.0f, "vc_compound_stitch: P_dB_norm_factor is 0");
    const float inv_norm = d_amp ? 1.0f / P_dB_norm_factor : 0.0f;
    const long long slab = (long long)out_frames * C;
    const int bf16 = src_dtype == VC_BF16;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (slab % 4) == 0 && aligned16(d_dst) && (!d_amp || aligned16(d_amp));
    if (vec && (C % 4) == 0 && aligned16(d_src))
        hipLaunchKernelGGL((compound_stitch_kernel<4, true>), dim3(tiles(slab, CT * 4), batch), dim3(CT), 0, st, d_src, bf16,
                           d_utt_tab, n_windows, T, C, out_frames, inv_norm, d_dst, d_amp);
    else if (vec)
        hipLaunchKernelGGL((compound_stitch_kernel<4, false>), dim3(tiles(slab, CT * 4), batch), dim3(CT), 0, st, d_src, bf16,
                           d_utt_tab, n_windows, T, C, out_frames, inv_norm, d_dst, d_amp);
    else
        hipLaunchKernelGGL((compound_stitch_kernel<1, false>), dim3(tiles(slab, CT), batch), dim3(CT), 0, st, d_src, bf16,
                           d_utt_tab, n_windows, T, C, out_frames, inv_norm, d_dst, d_amp);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_phase_init(const int32_t* d_n_frames, const int32_t* d_utt_id, int32_t batch, int32_t max_frames, int32_t n_bins,
                  int64_t seed, float* d_phase, void* stream) {
    VC_REQUIRE(d_phase, "vc_phase_init: NULL argument");
    VC_REQUIRE(batch > 0 && batch <= 65535 && max_frames > 0 && n_bins > 0, "vc_phase_init: bad shape (batch %d, max_frames %d, n_bins %d)",
               batch, max_frames, n_bins);
    const long long slab = (long long)max_frames * n_bins;
    VC_REQUIRE(slab < (1ll << 34), "vc_phase_init: an utterance holds more than 2^34 values (the Philox counter is e / 4 in 32 bits)");
    const dim3 grid(tiles((slab + 3) / 4, CT), batch);
    const uint32_t lo = (uint32_t)(uint64_t)seed, hi = (uint32_t)((uint64_t)seed >> 32);
    hipStream_t st = (hipStream_t)stream;
    if ((slab % 4) == 0 && aligned16(d_phase))
        hipLaunchKernelGGL((phase_init_kernel<true>), grid, dim3(CT), 0, st, d_n_frames, d_utt_id, max_frames, n_bins, lo, hi, d_phase);
    else
        hipLaunchKernelGGL((phase_init_kernel<false>), grid, dim3(CT), 0, st, d_n_frames, d_utt_id, max_frames, n_bins, lo, hi, d_phase);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
