// Deterministic Griffin-Lim phase start: single-pass spectrogram inversion (Beauregard, Harish & Wyse 2015) in the exact
// fixed-point form of include/vc_hip.h (vc_phase_spsi).  Phase is a uint32 fraction of a turn, addition wraps.
//
// Per frame the recurrence is a map  v(t, b) = v(t-1, q[b]) + w[b]  (q = owning peak or b itself, w = the peak's phase
// increment plus a half turn on odd neighbours, or 0).  Such maps compose associatively and, the offsets wrapping in
// uint32, exactly -- so the time axis is a scan over chunks of SPSI_CHUNK frames, in three launches:
//
//   spsi_compose_kernel  (chunk, utterance)  the chunk's map: (src uint16, off uint32)[nb]
//   spsi_scan_kernel     (utterance)         V[c+1][b] = V[c][src_c[b]] + off_c[b], V[0] = 0; every V[c] stored
//   spsi_replay_kernel   (chunk, utterance)  replays the chunk from V[c]; writes the phases, zeros beyond n_frames
//
// No workgroup waits for another inside a launch (no flags, no polling): order comes from the launches.  No atomics, no
// memset; every output element is written exactly once.
//
// All three work the same way: fill LDS tables (q uint16, w uint32)[S][nb] for S steps at once -- every entry is
// independent -- then walk the S steps.  compose walks backwards per bin (follow b through q of the last frame, then of
// the one before, ...: no barrier between steps); scan and replay walk forwards through a double-buffered V[nb] with one
// barrier per step.  compose and replay first copy the S rows of magnitudes into LDS (one coalesced pass: a single
// round trip to memory per fill) and search there: a search in global memory is a chain of two or three dependent
// loads per bin, and measured twice the time.  S is the chunk split evenly into as few fills as fit
// 64 KiB (no opt-in): two fills of 16 frames at nb = 201, 34.6 KB per workgroup.
//
// The owner search walks the rising, then the falling run from the bin; runs between spectral peaks are a few bins long.
// Every index is clamped by the loop bounds, never computed from a magnitude's value: any input bits give some phase.
#include "vc_device.h"

namespace {

constexpr int SPSI_CHUNK = 32;                 // frames per chunk (audio_lib.SPSI_CHUNK_FRAMES)
constexpr int ST = 512;                        // threads per workgroup
constexpr int LDS_BYTES = 65536;               // static-equivalent budget: no opt-in needed

// LDS: w_tab u32 [S * nb] | aux u32 [3 * nb] | q_tab u16 [S * nb] | (compose, replay) rows f32 [S * nb].  aux: compose --
// inc[nb], off state[nb], src state[nb]; scan -- V double buffer; replay -- inc[nb], V double buffer.
// Steps per fill: `want` steps split evenly into the fewest fills that fit; 0 if not even one step fits.
inline int spsi_steps(int nb, int want, int bytes_per_entry) {
    const long long most = ((long long)LDS_BYTES - 16 - 12ll * nb) / ((long long)bytes_per_entry * nb);   // 16: alignment slack
    if (most < 1) return 0;
    const long long fills = (want + most - 1) / most;
    return (int)((want + fills - 1) / fills);
}
inline size_t spsi_lds(int nb, int S, int bytes_per_entry) {
    return (((size_t)S * nb * 6 + (size_t)nb * 12 + 3) & ~(size_t)3) + (bytes_per_entry > 6 ? (size_t)S * nb * 4 : 0);
}

struct FrameMap { uint32_t q, w; };

// One entry of a frame's map.  m: the frame's nb magnitudes; inc_whole[k] = floor(((hop k) mod n_fft) 2^32 / n_fft).
__device__ __forceinline__ FrameMap frame_map(const float* m, int nb, int b, const uint32_t* inc_whole,
                                              double scale) {
    FrameMap r{(uint32_t)b, 0u};
    if (b < 1 || b > nb - 2) return r;
    const float mb = m[b];
    int k = -1;
    if (mb > m[b - 1] && mb > m[b + 1]) {
        k = b;
    } else {
        int j = b;
        float cur = mb, nxt = m[b + 1];
        while (cur < nxt) {                                        // rising run: ends at nb-1 at the latest
            ++j; cur = nxt;
            if (j == nb - 1) break;
            nxt = m[j + 1];
        }
        if (j > b && j <= nb - 2 && m[j] > m[j + 1]) {
            k = j;
        } else {
            j = b; cur = mb;
            float prv = m[b - 1];
            while (cur < prv) {                                    // falling run seen from above: ends at 0 at the latest
                --j; cur = prv;
                if (j == 0) break;
                prv = m[j - 1];
            }
            if (j < b && j >= 1 && m[j] > m[j - 1]) k = j;
        }
    }
    if (k < 0) return r;
    const float a = m[k - 1], c = m[k], d = m[k + 1];
    float p = (0.5f * (a - d)) / ((a - 2.0f * c) + d);
    if (!(fabsf(p) <= 1.0f)) p = 0.0f;                             // infinite or negative magnitudes only
    const uint32_t frac = (uint32_t)(unsigned long long)llrint((double)p * scale);
    r.q = (uint32_t)k;
    r.w = inc_whole[k] + frac + ((uint32_t)((b - k) & 1) << 31);
    return r;
}

__device__ __forceinline__ void fill_inc(uint32_t* inc, int nb, int n_fft, int hop) {
    for (int b = threadIdx.x; b < nb; b += ST)
        inc[b] = (uint32_t)(((((unsigned long long)hop * (unsigned)b) % (unsigned)n_fft) << 32) / (unsigned)n_fft);
}

// Tables of frames [lo, hi) of one utterance (amp_u: its [Fmax, nb] slab) through their copy in `rows`.  The caller
// barriers before (rows and tables free) and after (tables written).
__device__ __forceinline__ void fill_tables(const float* __restrict__ amp_u, int nb, int lo, int hi, const uint32_t* inc,
                                            double scale, float* rows, uint32_t* w_tab, uint16_t* q_tab) {
    const int n = (hi - lo) * nb;
    const float* src = amp_u + (size_t)lo * nb;
    for (int i = threadIdx.x; i < n; i += ST) rows[i] = src[i];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += ST) {
        const int f = i / nb, b = i - f * nb;
        const FrameMap e = frame_map(rows + f * nb, nb, b, inc, scale);
        w_tab[i] = e.w;
        q_tab[i] = (uint16_t)e.q;
    }
}

__device__ __forceinline__ int frames_of(const int32_t* n_frames, int u, int Fmax) {
    return min(max(n_frames ? n_frames[u] : Fmax, 0), Fmax);
}

// ---- 1: the map of chunk c of utterance u.  grid (chunks, B).  Chunks that start at or beyond n_frames write nothing
// (neither of the later launches reads them).
__global__ void __launch_bounds__(ST)
spsi_compose_kernel(const float* __restrict__ amp, const int32_t* __restrict__ n_frames, int Fmax, int nb, int n_fft, int hop,
                    double scale, int S, uint32_t* __restrict__ tab_off, uint16_t* __restrict__ tab_src) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int u = blockIdx.y, c = blockIdx.x;
    const int nf = frames_of(n_frames, u, Fmax);
    const int t0 = c * SPSI_CHUNK, t1 = min(t0 + SPSI_CHUNK, nf);
    if (t0 >= nf) return;
    uint32_t* w_tab = lds;
    uint32_t* inc = lds + (size_t)S * nb;
    uint32_t* st_off = inc + nb;
    uint32_t* st_src = st_off + nb;
    uint16_t* q_tab = reinterpret_cast<uint16_t*>(st_src + nb);
    float* rows = reinterpret_cast<float*>(lds + (((size_t)S * nb * 6 + (size_t)nb * 12 + 3) >> 2));
    const float* amp_u = amp + (size_t)u * Fmax * nb;
    fill_inc(inc, nb, n_fft, hop);
    for (int b = threadIdx.x; b < nb; b += ST) { st_off[b] = 0u; st_src[b] = (uint32_t)b; }   // own bins only
    __syncthreads();
    for (int hi = t1; hi > t0; hi -= S) {
        const int lo = max(t0, hi - S);
        fill_tables(amp_u, nb, lo, hi, inc, scale, rows, w_tab, q_tab);
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += ST) {
            uint32_t s = st_src[b], o = st_off[b];
            for (int t = hi - 1; t >= lo; --t) {
                const int i = (t - lo) * nb + (int)s;
                o += w_tab[i];
                s = q_tab[i];
            }
            st_src[b] = s; st_off[b] = o;
        }
        __syncthreads();
    }
    const size_t base = ((size_t)u * gridDim.x + c) * nb;
    for (int b = threadIdx.x; b < nb; b += ST) {
        tab_off[base + b] = st_off[b];
        tab_src[base + b] = (uint16_t)st_src[b];
    }
}

// ---- 2: the state at the start of every chunk.  grid (B).
__global__ void __launch_bounds__(ST)
spsi_scan_kernel(const int32_t* __restrict__ n_frames, int Fmax, int nb, int n_chunks, int S,
                 const uint32_t* __restrict__ tab_off, const uint16_t* __restrict__ tab_src, uint32_t* __restrict__ V) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int u = blockIdx.x;
    const int nf = frames_of(n_frames, u, Fmax);
    const int nck = (nf + SPSI_CHUNK - 1) / SPSI_CHUNK;            // chunks that hold a frame: V[0 .. nck-1] are read
    if (nck == 0) return;
    uint32_t* w_tab = lds;
    uint32_t* v0 = lds + (size_t)S * nb;
    uint32_t* v1 = v0 + nb;
    uint16_t* q_tab = reinterpret_cast<uint16_t*>(v1 + 2 * nb);
    const size_t base = (size_t)u * n_chunks * nb;
    for (int b = threadIdx.x; b < nb; b += ST) { v0[b] = 0u; V[base + b] = 0u; }
    for (int lo = 0; lo < nck - 1; lo += S) {
        const int hi = min(lo + S, nck - 1);
        const int n = (hi - lo) * nb;
        __syncthreads();                                           // the previous walk has read its tables
        for (int i = threadIdx.x; i < n; i += ST) {
            w_tab[i] = tab_off[base + (size_t)lo * nb + i];
            q_tab[i] = (uint16_t)min((int)tab_src[base + (size_t)lo * nb + i], nb - 1);
        }
        __syncthreads();
        for (int c = lo; c < hi; ++c) {
            const int row = (c - lo) * nb;
            for (int b = threadIdx.x; b < nb; b += ST) {
                const uint32_t v = v0[q_tab[row + b]] + w_tab[row + b];
                v1[b] = v;
                V[base + (size_t)(c + 1) * nb + b] = v;
            }
            __syncthreads();
            uint32_t* t = v0; v0 = v1; v1 = t;
        }
    }
}

// ---- 3: the phases of chunk c of utterance u.  grid (chunks, B).
__global__ void __launch_bounds__(ST)
spsi_replay_kernel(const float* __restrict__ amp, const int32_t* __restrict__ n_frames, int Fmax, int nb, int n_fft, int hop,
                   double scale, int S, const uint32_t* __restrict__ V, float* __restrict__ phase) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int u = blockIdx.y, c = blockIdx.x;
    const int nf = frames_of(n_frames, u, Fmax);
    const int t0 = c * SPSI_CHUNK, tend = min(t0 + SPSI_CHUNK, Fmax), t1 = min(tend, nf);
    float* out_u = phase + (size_t)u * Fmax * nb;
    {                                                              // rows beyond the utterance
        const int z0 = max(t0, nf);
        float* z = out_u + (size_t)z0 * nb;
        const int n = (tend - z0) * nb;
        for (int i = threadIdx.x; i < n; i += ST) z[i] = 0.0f;
    }
    if (t0 >= nf) return;
    uint32_t* w_tab = lds;
    uint32_t* inc = lds + (size_t)S * nb;
    uint32_t* v0 = inc + nb;
    uint32_t* v1 = v0 + nb;
    uint16_t* q_tab = reinterpret_cast<uint16_t*>(v1 + nb);
    float* rows = reinterpret_cast<float*>(lds + (((size_t)S * nb * 6 + (size_t)nb * 12 + 3) >> 2));
    const float* amp_u = amp + (size_t)u * Fmax * nb;
    const size_t vbase = ((size_t)u * gridDim.x + c) * nb;
    fill_inc(inc, nb, n_fft, hop);
    for (int b = threadIdx.x; b < nb; b += ST) v0[b] = V[vbase + b];
    for (int lo = t0; lo < t1; lo += S) {
        const int hi = min(lo + S, t1);
        __syncthreads();                                           // inc and v0 written; the previous walk has read its tables
        fill_tables(amp_u, nb, lo, hi, inc, scale, rows, w_tab, q_tab);
        __syncthreads();
        for (int t = lo; t < hi; ++t) {
            const int row = (t - lo) * nb;
            float* o = out_u + (size_t)t * nb;
            for (int b = threadIdx.x; b < nb; b += ST) {
                const uint32_t v = v0[q_tab[row + b]] + w_tab[row + b];
                v1[b] = v;
                o[b] = __fmul_rn((float)(int32_t)v, 1.4629180792671596e-9f);   // float32(pi / 2^31)
            }
            __syncthreads();
            uint32_t* s = v0; v0 = v1; v1 = s;
        }
    }
}

inline int n_chunks_of(int max_frames) { return (max_frames + SPSI_CHUNK - 1) / SPSI_CHUNK; }

}  // namespace

extern "C" {

size_t vc_phase_spsi_workspace_bytes(int32_t batch, int32_t max_frames, int32_t n_bins) {
    if (batch <= 0 || max_frames <= 0 || n_bins <= 0) return 0;
    const size_t e = (size_t)batch * n_chunks_of(max_frames) * n_bins;
    return vc::align256(e * 4) + vc::align256(e * 4) + vc::align256(e * 2);     // chunk offsets, V, chunk sources
}

int vc_phase_spsi(const float* d_amp, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_bins,
                  int32_t n_fft, int32_t hop, float* d_phase, void* d_workspace, size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_amp && d_phase && d_workspace, "vc_phase_spsi: NULL argument");
    VC_REQUIRE(batch > 0 && batch <= 65535 && max_frames > 0, "vc_phase_spsi: bad shape (batch %d, max_frames %d)", batch, max_frames);
    VC_REQUIRE(n_fft >= 4 && n_bins == 1 + n_fft / 2, "vc_phase_spsi: n_fft %d must be >= 4 and n_bins %d must be 1 + n_fft/2", n_fft,
               n_bins);
    VC_REQUIRE(n_bins <= 65535, "vc_phase_spsi: n_bins %d exceeds 65535 (chunk maps hold uint16 bin indices)", n_bins);
    VC_REQUIRE(hop > 0 && hop <= 65535, "vc_phase_spsi: hop %d must be in [1, 65535]", hop);
    const int S = spsi_steps(n_bins, SPSI_CHUNK, 10);               // compose, replay: tables and rows
    VC_REQUIRE(S >= 1, "vc_phase_spsi: n_bins %d does not fit the kernels' LDS tables (22 bytes per bin in 64 KiB: at most 2978)",
               n_bins);
    const int nck = n_chunks_of(max_frames);
    VC_REQUIRE((long long)max_frames * n_bins < (1ll << 31) && (long long)nck * n_bins < (1ll << 31), "vc_phase_spsi: too large");
    VC_REQUIRE(workspace_bytes >= vc_phase_spsi_workspace_bytes(batch, max_frames, n_bins),
               "vc_phase_spsi: workspace of %zu bytes, vc_phase_spsi_workspace_bytes asks for %zu", workspace_bytes,
               vc_phase_spsi_workspace_bytes(batch, max_frames, n_bins));
    VC_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 3) == 0, "vc_phase_spsi: workspace must be 4-byte aligned");
    const size_t e = (size_t)batch * nck * n_bins;
    char* ws = static_cast<char*>(d_workspace);
    uint32_t* tab_off = reinterpret_cast<uint32_t*>(ws);
    uint32_t* V = reinterpret_cast<uint32_t*>(ws + vc::align256(e * 4));
    uint16_t* tab_src = reinterpret_cast<uint16_t*>(ws + 2 * vc::align256(e * 4));
    const double scale = (double)hop * 4294967296.0 / (double)n_fft;
    const int S_scan = spsi_steps(n_bins, nck > 1 ? nck - 1 : 1, 6);   // scan: tables only, all chunk maps at once if they fit
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(spsi_compose_kernel, dim3(nck, batch), dim3(ST), spsi_lds(n_bins, S, 10), st, d_amp, d_n_frames, max_frames,
                       n_bins, n_fft, hop, scale, S, tab_off, tab_src);
    hipLaunchKernelGGL(spsi_scan_kernel, dim3(batch), dim3(ST), spsi_lds(n_bins, S_scan, 6), st, d_n_frames, max_frames, n_bins, nck,
                       S_scan, tab_off, tab_src, V);
    hipLaunchKernelGGL(spsi_replay_kernel, dim3(nck, batch), dim3(ST), spsi_lds(n_bins, S, 10), st, d_amp, d_n_frames, max_frames,
                       n_bins, n_fft, hop, scale, S, V, d_phase);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
