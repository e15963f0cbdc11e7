// Harmonic-plus-noise vocoder (include/vc_hip.h, "Harmonic-plus-noise vocoder"): envelope and F0 in, waveform out.
//
//   env_cepstral_kernel    amp [B, F, nb] -> env_log, theta [B, F, nb]: the true-envelope iteration on a cepstrum of order L
//                          and the minimum phase of the result.  A workgroup owns up to 8 consecutive frames of one
//                          utterance; the cos / sin table, the frames' log magnitudes and their cepstra live in LDS.
//   hnm_plan_kernel        f0 [B, F] -> voiced, inc, slope, phase, flags: integers only.  One workgroup per utterance walks
//                          the frames in tiles of 256: a maximum scan carries the last voiced frame, a wrapping sum scan the
//                          phase.
//   noise_init_kernel      (seed, utt_id, sample) -> unit-variance uniform noise [B, Lmax], Philox4x32-10 as vc_phase_init.
//   noise_gain_kernel      env_log, voiced -> the gain that shapes that noise through vc_stft_filter_f32.
//   hnm_synth_kernel       env_log, theta, the plan -> y [B, hop (F - 1)]: grid (tiles of 16 intervals, B).  A tile first
//                          writes (a_e[k], t_e[k]) for its 17 frames and up to 256 harmonics into LDS -- the exponentials
//                          are per frame, not per sample -- then every lane takes samples and loops over the harmonics.
//
// Every count is read on the device and clamped; nothing read from a table forms an address unclamped; no atomics, every
// output element is written once.
#include "vc_common.h"
#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int MAX_F = 16384;            // WARP_MAX_FRAMES
constexpr int MAX_NFFT = 2048, MAX_HOP = 4096;
constexpr int ENV_FRAMES = 8;           // frames per workgroup of the envelope kernel, fewer where LDS runs out
constexpr size_t ENV_LDS = 64 * 1024;
constexpr int HNM_MAX_HARMONICS = 256;
constexpr int TI = 16;                  // intervals per tile of the synthesis kernel
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float INV_2PI = 0.15915494309189533577f;
constexpr float TWO_M32 = 2.3283064365386962890625e-10f;

__device__ __forceinline__ int clamp_frames(const int32_t* n_frames, int b, int F) {
    return min(max(n_frames ? n_frames[b] : F, 0), F);
}

// ---- envelope.  LDS: T[N] (cos, sin) | a[fpb][nb] | A[fpb][nb] | c[fpb][L + 1]
__global__ void __launch_bounds__(NT)
env_cepstral_kernel(const float* __restrict__ amp, const int32_t* __restrict__ n_frames, const float2* __restrict__ tab, int F,
                    int N, int L, int passes, float floor_v, int fpb, float* __restrict__ env_log, float* __restrict__ theta) {
    extern __shared__ float4 env_smem[];
    const int nb = N / 2 + 1, L1 = L + 1;
    float2* T = reinterpret_cast<float2*>(env_smem);
    float* a = reinterpret_cast<float*>(env_smem) + 2 * N;
    float* A = a + fpb * nb;
    float* c = A + fpb * nb;
    const int t = threadIdx.x, b = blockIdx.y;
    const int f0 = blockIdx.x * fpb;
    const int nf = min(fpb, F - f0);
    const int nlive = min(max(clamp_frames(n_frames, b, F) - f0, 0), nf);
    const size_t base = ((size_t)b * F + f0) * nb;
    for (int i = nlive * nb + t; i < nf * nb; i += NT) { env_log[base + i] = 0.0f; theta[base + i] = 0.0f; }
    if (nlive == 0) return;
    for (int i = t; i < N; i += NT) T[i] = tab[i];
    for (int i = t; i < nlive * nb; i += NT) {
        const float v = logf(fmaxf(amp[base + i], floor_v));
        a[i] = v;
        A[i] = v;
    }
    __syncthreads();
    const float invN = 1.0f / (float)N;
    const int half = N / 2;
    for (int p = 0; p < passes; ++p) {
        for (int i = t; i < nlive * L1; i += NT) {                  // c_n: one lane per (frame, n), k ascending
            const int f = i / L1, n = i - f * L1;
            const float* Af = A + f * nb;
            float acc = 0.0f;
            int idx = n;
            for (int k = 1; k < half; ++k) {
                acc = fmaf(Af[k], T[idx].x, acc);
                idx += n;
                if (idx >= N) idx -= N;
            }
            const float edge = fmaf(T[idx].x, Af[half], Af[0]);     // T[(n N / 2) mod N].x = (-1)^n
            c[i] = fmaf(2.0f, acc, edge) * invN;
        }
        __syncthreads();
        const bool last = p == passes - 1;
        for (int i = t; i < nlive * nb; i += NT) {                  // E_k, theta_k: one lane per (frame, k), n ascending
            const int f = i / nb, k = i - f * nb;
            const float* cf = c + f * L1;
            float e = 0.0f, th = 0.0f;
            int idx = k;
            for (int n = 1; n <= L; ++n) {
                const float2 tw = T[idx];
                e = fmaf(cf[n], tw.x, e);
                th = fmaf(cf[n], tw.y, th);
                idx += k;
                if (idx >= N) idx -= N;
            }
            const float E = fmaf(2.0f, e, cf[0]);
            if (last) {
                env_log[base + i] = E;
                theta[base + i] = -2.0f * th;
            } else {
                A[i] = fmaxf(a[i], E);
            }
        }
        __syncthreads();
    }
}

// ---- plan
__device__ __forceinline__ bool f0_voiced(float x, float lo, float hi) { return x >= lo && x <= hi; }   // false for NaN
__device__ __forceinline__ uint32_t f0_inc(float x, float kinc) { return (uint32_t)rintf(__fmul_rn(x, kinc)); }

// Exclusive wrapping sum over the workgroup (4 waves); two barriers, every lane calls it.
__device__ inline uint32_t scan_excl_u32(uint32_t v, uint32_t* wtot, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t u = __shfl_up(inc, s, 64);
        if (lane >= s) inc += u;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t off = 0, all = 0;
    for (int w = 0; w < NT / 64; ++w) {
        const uint32_t x = wtot[w];
        if (w < wave) off += x;
        all += x;
    }
    total = all;
    return inc - v + off;
}

__global__ void __launch_bounds__(NT)
hnm_plan_kernel(const float* __restrict__ f0, const int32_t* __restrict__ n_frames, int F, int hop, float kinc, float f0_lo,
                float f0_hi, uint8_t* __restrict__ voiced, uint32_t* __restrict__ inc, int32_t* __restrict__ slope,
                uint32_t* __restrict__ phase, int32_t* __restrict__ flags) {
    __shared__ int wmax[NT / 64];
    __shared__ uint32_t wsum[NT / 64];
    __shared__ int wfirst[NT / 64];
    const int t = threadIdx.x, b = blockIdx.x;
    const int nF = clamp_frames(n_frames, b, F);
    const size_t row = (size_t)b * F;
    const float* x = f0 + row;
    int first = F, bad = 0;
    for (int f = t; f < F; f += NT) {
        bool v = false;
        if (f < nF) {
            const float xv = x[f];
            v = f0_voiced(xv, f0_lo, f0_hi);
            if (!v && xv != 0.0f) bad = 1;                          // NaN included
            if (v) first = min(first, f);
        }
        voiced[row + f] = v ? 1 : 0;
    }
    bad = __syncthreads_or(bad);
    if (t == 0) flags[b] = bad ? 1 : 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) first = min(first, __shfl_xor(first, s, 64));
    if ((t & 63) == 0) wfirst[t >> 6] = first;
    __syncthreads();
    first = min(min(wfirst[0], wfirst[1]), min(wfirst[2], wfirst[3]));
    const uint32_t inc_lead = first < F ? f0_inc(x[first], kinc) : 0u;      // a leading unvoiced run; 0: no voiced frame
    const uint32_t hh = (uint32_t)(((unsigned long long)hop * (unsigned)(hop - 1)) >> 1);
    int carry_last = -1;
    uint32_t carry_phase = 0;
    for (int f_base = 0; f_base < F; f_base += NT) {
        const int f = f_base + t;
        const bool in = f < nF;
        const int own = (in && f0_voiced(x[f], f0_lo, f0_hi)) ? f : -1;
        int total;
        const int last = max(max(vc::block_scan_excl<false, NT / 64>(own, wmax, total), own), carry_last);
        carry_last = max(carry_last, total);
        uint32_t iv = 0, step = 0;
        int sl = 0;
        if (in) {
            iv = last >= 0 ? f0_inc(x[last], kinc) : inc_lead;
            if (f + 1 < nF) {
                const int last1 = f0_voiced(x[f + 1], f0_lo, f0_hi) ? f + 1 : last;
                const uint32_t iv1 = last1 >= 0 ? f0_inc(x[last1], kinc) : inc_lead;
                const long long d = (long long)iv1 - (long long)iv;
                long long q = d / hop;
                if (d < 0 && q * hop != d) --q;                     // floor
                sl = (int)q;
            }
            step = (uint32_t)hop * iv + (uint32_t)sl * hh;
        }
        uint32_t tile_sum;
        const uint32_t ph = carry_phase + scan_excl_u32(step, wsum, tile_sum);
        carry_phase += tile_sum;
        if (f < F) {
            inc[row + f] = iv;
            slope[row + f] = sl;
            phase[row + f] = in ? ph : 0u;
        }
    }
}

// ---- noise
__global__ void __launch_bounds__(NT)
noise_init_kernel(const int32_t* __restrict__ lens, const int32_t* __restrict__ utt_id, int Lmax, uint32_t seed_lo,
                  uint32_t seed_hi, float* __restrict__ noise) {
    const int b = blockIdx.y;
    const long long e0 = ((long long)blockIdx.x * NT + threadIdx.x) * 4;
    if (e0 >= Lmax) return;
    const int len = min(max(lens ? lens[b] : Lmax, 0), Lmax);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e0 < len) {
        uint32_t x[4];
        vc::philox4x32_10((uint32_t)(e0 >> 2), (uint32_t)(utt_id ? utt_id[b] : b), 0u, 0u, seed_lo, seed_hi, x);
#pragma unroll
        for (int k = 0; k < 4; ++k)                                 // (x >> 8) * 2^-24 - 0.5 is exact: one rounding
            v[k] = (e0 + k < len) ? __fmul_rn(3.46410161513775458705f, (float)(x[k] >> 8) * 5.9604644775390625e-8f - 0.5f) : 0.0f;
    }
    float* o = noise + (size_t)b * Lmax;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e0 + k < Lmax) o[e0 + k] = v[k];
}

__global__ void __launch_bounds__(NT)
noise_gain_kernel(const float* __restrict__ env_log, const uint8_t* __restrict__ voiced, const int32_t* __restrict__ n_frames,
                  int F, int nb, int cutoff_bin, float gscale, float* __restrict__ G) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= F * nb) return;
    const int f = i / nb, k = i - f * nb;
    const size_t at = (size_t)b * F * nb + i;
    float g = 0.0f;
    if (f < clamp_frames(n_frames, b, F) && (!voiced[(size_t)b * F + f] || k >= cutoff_bin))
        g = gscale * exp2f(env_log[at] * LOG2E);
    G[at] = g;
}

// ---- synthesis
// cos(2 pi x): x - rint(x) is exact; z = 1/4 - |x| in [-1/4, 1/4]; sin(2 pi z) as z times a polynomial in z^2 (a least-squares
// fit at Chebyshev nodes, float32 coefficients: 3.1e-8 from sin(2 pi z) over the interval, tests/test_hnm_cpu.py).
__device__ __forceinline__ float cos_turns(float x) {
    x = x - rintf(x);
    const float z = 0.25f - fabsf(x);
    const float s = z * z;
    float p = fmaf(s, 39.76072311401367f, -76.58128356933594f);
    p = fmaf(s, p, 81.60247802734375f);
    p = fmaf(s, p, -41.34168243408203f);
    p = fmaf(s, p, 6.2831854820251465f);
    return z * p;
}

__device__ __forceinline__ float lerp_row(const float* __restrict__ r, int i0, int i1, float fr) {
    const float v = r[i0];
    return fmaf(fr, r[i1] - v, v);
}

__global__ void __launch_bounds__(NT)
hnm_synth_kernel(const float* __restrict__ env_log, const float* __restrict__ theta, const uint8_t* __restrict__ voiced,
                 const uint32_t* __restrict__ inc, const int32_t* __restrict__ slope, const uint32_t* __restrict__ phase,
                 const int32_t* __restrict__ n_frames, const float* __restrict__ add, int F, int N, int hop, uint32_t cutoff_inc,
                 float scale, float* __restrict__ y) {
    __shared__ float2 tab[TI + 1][HNM_MAX_HARMONICS];               // (a_e[k], t_e[k]) at [e][k - 1]; (0, 0) for a dead end
    __shared__ int Ke[TI + 1];
    __shared__ uint32_t s_inc[TI + 1], s_ph[TI + 1];
    __shared__ int s_sl[TI + 1];
    const int t = threadIdx.x, b = blockIdx.y;
    const int i0 = blockIdx.x * TI;
    const int nb = N / 2 + 1;
    const int ni = min(TI, F - 1 - i0);
    const int nlive = min(max(clamp_frames(n_frames, b, F) - 1 - i0, 0), ni);
    const size_t L = (size_t)hop * (F - 1);
    const size_t at0 = (size_t)b * L + (size_t)i0 * hop;
    if (nlive == 0) {
        for (int s = t; s < ni * hop; s += NT) y[at0 + s] = 0.0f;
        return;
    }
    const size_t frow = (size_t)b * F + i0;
    if (t <= nlive) {
        const uint32_t ic = inc[frow + t];
        Ke[t] = (voiced[frow + t] && ic > 0u) ? (int)min((cutoff_inc - 1u) / ic, (uint32_t)HNM_MAX_HARMONICS) : 0;
        s_inc[t] = ic;
        s_ph[t] = phase[frow + t];
        s_sl[t] = slope[frow + t];
    }
    __syncthreads();
    for (int i = t; i < (nlive + 1) * HNM_MAX_HARMONICS; i += NT) {
        const int e = i / HNM_MAX_HARMONICS, k = i - e * HNM_MAX_HARMONICS + 1;
        float2 v = make_float2(0.0f, 0.0f);
        if (k <= Ke[e]) {
            const unsigned long long q = (unsigned long long)((uint32_t)k * s_inc[e]) * (unsigned)N;   // k inc < cutoff_inc
            const int bin = min((int)(q >> 32), nb - 1), bin1 = min(bin + 1, nb - 1);
            const float fr = (float)(uint32_t)q * TWO_M32;
            const size_t r = (frow + e) * nb;
            v.x = scale * exp2f(lerp_row(env_log + r, bin, bin1, fr) * LOG2E);
            v.y = lerp_row(theta + r, bin, bin1, fr);
        }
        tab[e][k - 1] = v;
    }
    __syncthreads();
    const float fhop = (float)hop;
    for (int s = t; s < ni * hop; s += NT) {
        const int il = s / hop, j = s - il * hop;
        float out = 0.0f;
        if (il < nlive) {
            const int K0 = Ke[il], K1 = Ke[il + 1], K = max(K0, K1);
            const float u = __fdiv_rn((float)j, fhop);
            const uint32_t phi = s_ph[il] + (uint32_t)j * s_inc[il] + (uint32_t)s_sl[il] * (uint32_t)((j * (j - 1)) >> 1);
            const float2* T0 = tab[il];
            const float2* T1 = tab[il + 1];
            float acc = 0.0f;
            uint32_t kphi = 0;
            for (int k = 1; k <= K; ++k) {
                kphi += phi;
                const float2 A0 = T0[k - 1], A1 = T1[k - 1];
                const float t0 = k <= K0 ? A0.y : A1.y, t1 = k <= K1 ? A1.y : A0.y;
                const float a = fmaf(u, A1.x - A0.x, A0.x);
                const float tt = fmaf(u, t1 - t0, t0);
                const float xturn = fmaf(tt, INV_2PI, (float)(int32_t)kphi * TWO_M32);
                acc = fmaf(a, cos_turns(xturn), acc);
            }
            out = acc;
            if (add) {
                const float av = add[at0 + s];
                out = K > 0 ? acc + av : av;
            }
        }
        y[at0 + s] = out;
    }
}

inline bool finite_pos(float v) { return std::isfinite(v) && v > 0.0f; }
inline int env_fpb(int N, int L) {
    const size_t fixed = (size_t)2 * N * sizeof(float), per = ((size_t)2 * (N / 2 + 1) + L + 1) * sizeof(float);
    return (int)std::min<size_t>(ENV_FRAMES, (ENV_LDS - fixed) / per);
}

}  // namespace

extern "C" {

int32_t vc_hnm_max_harmonics(void) { return HNM_MAX_HARMONICS; }
int32_t vc_hnm_tile_intervals(void) { return TI; }

int vc_env_cepstral_f32(const float* d_amp, const int32_t* d_n_frames, const float* d_table, int32_t batch, int32_t max_frames,
                        int32_t n_fft, int32_t order, int32_t iters, float floor, float* d_env_log, float* d_theta,
                        void* stream) {
    VC_REQUIRE(d_amp && d_table && d_env_log && d_theta, "vc_env_cepstral_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1, "vc_env_cepstral_f32: bad shape (batch %d, max_frames %d)", batch, max_frames);
    VC_REQUIRE(n_fft >= 4 && (n_fft % 2) == 0 && order >= 1 && order < n_fft / 2 && iters >= 0,
               "vc_env_cepstral_f32: need n_fft even and >= 4, 1 <= order < n_fft / 2, iters >= 0 (got %d, %d, %d)", n_fft, order,
               iters);
    VC_REQUIRE(finite_pos(floor), "vc_env_cepstral_f32: floor must be positive and finite");
    VC_REQUIRE(d_amp != d_env_log && d_amp != d_theta && d_env_log != d_theta, "vc_env_cepstral_f32: not in place");
    if (batch > 65535 || max_frames > MAX_F || n_fft > MAX_NFFT || iters > 1024)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_env_cepstral_f32: limits are batch <= 65535, max_frames <= %d, n_fft <= %d "
                             "and iters <= 1024; got batch %d, max_frames %d, n_fft %d, iters %d", MAX_F, MAX_NFFT, batch,
                             max_frames, n_fft, iters);
    const int fpb = env_fpb(n_fft, order);                          // >= 1 at every size within the limits
    const size_t smem = ((size_t)2 * n_fft + (size_t)fpb * (2 * (n_fft / 2 + 1) + order + 1)) * sizeof(float);
    hipLaunchKernelGGL(env_cepstral_kernel, dim3((max_frames + fpb - 1) / fpb, batch), dim3(NT), smem,
                       static_cast<hipStream_t>(stream), d_amp, d_n_frames, reinterpret_cast<const float2*>(d_table), max_frames,
                       n_fft, order, iters + 1, floor, fpb, d_env_log, d_theta);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_hnm_plan(const float* d_f0, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t sr, int32_t hop,
                float f0_lo, float f0_hi, uint8_t* d_voiced, uint32_t* d_inc, int32_t* d_slope, uint32_t* d_phase,
                int32_t* d_flags, void* stream) {
    VC_REQUIRE(d_f0 && d_voiced && d_inc && d_slope && d_phase && d_flags, "vc_hnm_plan: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && sr >= 1 && hop >= 1, "vc_hnm_plan: bad shape (batch %d, max_frames %d, sr %d, "
               "hop %d)", batch, max_frames, sr, hop);
    VC_REQUIRE(finite_pos(f0_lo) && std::isfinite(f0_hi) && f0_lo <= f0_hi && (double)f0_hi <= 0.5 * sr,
               "vc_hnm_plan: need 0 < f0_lo <= f0_hi <= sr / 2 (got %g, %g)", (double)f0_lo, (double)f0_hi);
    if (batch > 65535 || max_frames > MAX_F || hop > MAX_HOP)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_hnm_plan: limits are batch <= 65535, max_frames <= %d and hop <= %d; got "
                             "batch %d, max_frames %d, hop %d", MAX_F, MAX_HOP, batch, max_frames, hop);
    const float kinc = (float)(4294967296.0 / (double)sr);
    hipLaunchKernelGGL(hnm_plan_kernel, dim3(batch), dim3(NT), 0, static_cast<hipStream_t>(stream), d_f0, d_n_frames, max_frames,
                       hop, kinc, f0_lo, f0_hi, d_voiced, d_inc, d_slope, d_phase, d_flags);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_noise_init_f32(const int32_t* d_lens, const int32_t* d_utt_id, int32_t batch, int32_t max_len, int64_t seed,
                      float* d_noise, void* stream) {
    VC_REQUIRE(d_noise, "vc_noise_init_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_len >= 1, "vc_noise_init_f32: bad shape (batch %d, max_len %d)", batch, max_len);
    const uint32_t lo = (uint32_t)(uint64_t)seed, hi = (uint32_t)((uint64_t)seed >> 32);
    hipLaunchKernelGGL(noise_init_kernel, dim3((unsigned)(((long long)max_len + 4 * NT - 1) / (4 * NT)), batch), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), d_lens, d_utt_id, max_len, lo, hi, d_noise);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_hnm_noise_gain_f32(const float* d_env_log, const uint8_t* d_voiced, const int32_t* d_n_frames, int32_t batch,
                          int32_t max_frames, int32_t n_bins, int32_t cutoff_bin, float gscale, float* d_gain, void* stream) {
    VC_REQUIRE(d_env_log && d_voiced && d_gain, "vc_hnm_noise_gain_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_bins >= 1 && cutoff_bin >= 0, "vc_hnm_noise_gain_f32: bad shape (batch %d, "
               "max_frames %d, n_bins %d, cutoff_bin %d)", batch, max_frames, n_bins, cutoff_bin);
    VC_REQUIRE(std::isfinite(gscale) && gscale >= 0.0f, "vc_hnm_noise_gain_f32: gscale must be finite and not negative");
    if (batch > 65535 || max_frames > MAX_F || n_bins > MAX_NFFT / 2 + 1)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_hnm_noise_gain_f32: limits are batch <= 65535, max_frames <= %d and n_bins "
                             "<= %d; got batch %d, max_frames %d, n_bins %d", MAX_F, MAX_NFFT / 2 + 1, batch, max_frames, n_bins);
    hipLaunchKernelGGL(noise_gain_kernel, dim3((max_frames * n_bins + NT - 1) / NT, batch), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), d_env_log, d_voiced, d_n_frames, max_frames, n_bins, cutoff_bin, gscale,
                       d_gain);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_hnm_synth_f32(const float* d_env_log, const float* d_theta, const uint8_t* d_voiced, const uint32_t* d_inc,
                     const int32_t* d_slope, const uint32_t* d_phase, const int32_t* d_n_frames, const float* d_add,
                     int32_t batch, int32_t max_frames, int32_t n_fft, int32_t hop, int64_t cutoff_inc, float scale, float* d_y,
                     void* stream) {
    VC_REQUIRE(d_env_log && d_theta && d_voiced && d_inc && d_slope && d_phase && d_y, "vc_hnm_synth_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 2 && n_fft >= 4 && (n_fft % 2) == 0 && hop >= 1, "vc_hnm_synth_f32: bad shape (batch "
               "%d, max_frames %d (>= 2), n_fft %d (even, >= 4), hop %d)", batch, max_frames, n_fft, hop);
    VC_REQUIRE(cutoff_inc >= 1 && cutoff_inc <= 0x80000000ll, "vc_hnm_synth_f32: cutoff_inc must be in [1, 2^31] (Nyquist)");
    VC_REQUIRE(std::isfinite(scale) && scale >= 0.0f, "vc_hnm_synth_f32: scale must be finite and not negative");
    VC_REQUIRE(d_add != d_y, "vc_hnm_synth_f32: not in place");
    if (batch > 65535 || max_frames > MAX_F || n_fft > MAX_NFFT || hop > MAX_HOP)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_hnm_synth_f32: limits are batch <= 65535, max_frames <= %d, n_fft <= %d and "
                             "hop <= %d; got batch %d, max_frames %d, n_fft %d, hop %d", MAX_F, MAX_NFFT, MAX_HOP, batch,
                             max_frames, n_fft, hop);
    hipLaunchKernelGGL(hnm_synth_kernel, dim3((max_frames - 1 + TI - 1) / TI, batch), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), d_env_log, d_theta, d_voiced, d_inc, d_slope, d_phase, d_n_frames, d_add,
                       max_frames, n_fft, hop, (uint32_t)cutoff_inc, scale, d_y);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
