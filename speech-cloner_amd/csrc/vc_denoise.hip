// Noise suppression (include/vc_hip.h, "Noise suppression"): the noise tracker of Gerkmann & Hendriks (speech-presence
// probability under a fixed prior SNR) and the suppression rule (Wiener or Ephraim-Malah's log-MMSE on the
// decision-directed a-priori SNR) in ONE scan over the frames of P [B, maxF, bins] float32.
//
// Both are recursions along time and independent across bins and utterances, so one lane takes one (utterance, bin) and
// walks its frames; adjacent lanes take adjacent bins, so a wave reads and writes 64 consecutive floats of a row.  grid
// (64-bin groups, B), one wave a workgroup.  The chain per frame -- at log-MMSE three exponentials, a logarithm and seven
// divisions, serial through A = G^2 y of the frame before -- is what the launch costs: it is latency-bound by design, like
// the plan kernels of vc_pitch.hip and vc_wsola.hip.  The loads of P do not depend on the chain, so a lane keeps the next
// NG_PF frames in registers while it works on the current ones, and whole groups of NG_PF frames are straight-line code.
//
// float32 throughout, no contraction: every product and every sum below is rounded once, divisions are IEEE.  No atomics,
// no allocation, no host wait; n_frames is clamped to [0, maxF] when read; a lane beyond n_bins does nothing.
#include <cfloat>
#include <cmath>
#include <type_traits>
#include "vc_common.h"

namespace {

constexpr int NG_PF = 8;                // frames a lane holds ahead of the chain

struct NgArgs {
    const float* power;      // [B][maxF][nb]
    const int32_t* n_frames; // [B] or null
    const float* noise0;     // [B][nb] or null
    float* gain;             // [B][maxF][nb]
    float* noise;            // [B][maxF][nb] or null
    int maxF, nb;
    vc_denoise_cfg cfg;
};

// E1(x), x > 0: Abramowitz & Stegun 5.1.53 on x <= 1, 5.1.56 above, Horner form.  Both forms are evaluated (each on its own
// side of 1, so neither sees an argument it was not made for) and one is selected: the lanes of a wave sit on both sides
// anyway, and without a branch the two chains overlap
__device__ __forceinline__ float expint1(float x) {
#pragma clang fp contract(off)
    const float xs = fminf(x, 1.0f), xl = fmaxf(x, 1.0f);
    float q = 0.00107857f;
    q = q * xs + -0.00976004f;
    q = q * xs + 0.05519968f;
    q = q * xs + -0.24991055f;
    q = q * xs + 0.99999193f;
    q = q * xs + -0.57721566f;
    const float small = q - logf(xs);
    float n = xl + 8.5733287401f;
    n = n * xl + 18.0590169730f;
    n = n * xl + 8.6347608925f;
    n = n * xl + 0.2677737343f;
    float d = xl + 9.5733223454f;
    d = d * xl + 25.6329561486f;
    d = d * xl + 21.0996530827f;
    d = d * xl + 3.9584969228f;
    const float large = (expf(-xl) / xl) * (n / d);
    return x <= 1.0f ? small : large;
}

template <int RULE, bool NOISE>
__global__ void __launch_bounds__(64)
noise_gain_kernel(NgArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (k >= a.nb) return;
    const int maxF = a.maxF;
    const size_t nb = (size_t)a.nb;
    const int F = a.n_frames ? min(max(a.n_frames[b], 0), maxF) : maxF;
    const size_t base = (size_t)b * maxF * nb + k;
    const float* __restrict__ P = a.power + base;
    float* __restrict__ G = a.gain + base;
    float* __restrict__ S = NOISE ? a.noise + base : nullptr;

    const vc_denoise_cfg c = a.cfg;
    const float k1 = 1.0f + c.xi_h1, c1 = c.xi_h1 / k1;
    const float q_spp = 1.0f - c.a_spp, q_n = 1.0f - c.a_noise, q_dd = 1.0f - c.a_dd;

    if (F > 0) {
        float s;
        if (a.noise0) {
            s = a.noise0[(size_t)b * nb + k];
        } else {
            const int n0 = min(c.n_init, F);
            float acc = 0.0f;
            for (int f = 0; f < n0; ++f) acc = acc + P[(size_t)f * nb];
            s = acc / (float)n0;
        }
        s = fmaxf(s, FLT_MIN);
        float pb = 0.5f, A = 0.0f;
        float cur[NG_PF], nxt[NG_PF];
        // a frame index is clamped into [0, F) instead of guarded: a load that nobody uses costs nothing, a branch between
        // two frames would keep the scheduler from running the tracker of frame f + 1 under the gain of frame f
#pragma unroll
        for (int j = 0; j < NG_PF; ++j) cur[j] = P[(size_t)min(j, F - 1) * nb];
        int f0 = 0;
        // GUARD: the last, partial group of frames; the whole groups before it are straight-line code
        auto group = [&](auto guard) {
            constexpr bool GUARD = decltype(guard)::value;
#pragma unroll
            for (int j = 0; j < NG_PF; ++j) nxt[j] = P[(size_t)min(f0 + NG_PF + j, F - 1) * nb];
#pragma unroll
            for (int j = 0; j < NG_PF; ++j) {
                const int f = f0 + j;
                if (!GUARD || f < F) {
                    const float y = cur[j];
                    const float t = fminf((y / s) * c1, 80.0f);
                    float p = 1.0f / (1.0f + k1 * expf(-t));
                    pb = c.a_spp * pb + q_spp * p;
                    if (pb > 0.99f) p = fminf(p, 0.99f);
                    const float e = (1.0f - p) * y + p * s;
                    s = fmaxf(c.a_noise * s + q_n * e, FLT_MIN);
                    const float g = fminf(y / s, c.gamma_max);
                    const float r = f == 0 ? 1.0f : fminf(A / s, c.gamma_max);
                    const float xi = fmaxf(c.a_dd * r + q_dd * fmaxf(g - 1.0f, 0.0f), c.xi_min);
                    const float w = xi / (1.0f + xi);
                    float gn = w;
                    if (RULE == 1) gn = w * expf(0.5f * expint1(fmaxf(w * g, 1e-6f)));
                    gn = fminf(fmaxf(gn, c.gain_min), 1.0f);
                    A = (gn * gn) * y;
                    G[(size_t)f * nb] = gn;
                    if (NOISE) S[(size_t)f * nb] = s;
                }
            }
#pragma unroll
            for (int j = 0; j < NG_PF; ++j) cur[j] = nxt[j];
        };
        for (; f0 + NG_PF <= F; f0 += NG_PF) group(std::false_type{});
        if (f0 < F) group(std::true_type{});
    }
    for (int f = F; f < maxF; ++f) {
        G[(size_t)f * nb] = 0.0f;
        if (NOISE) S[(size_t)f * nb] = 0.0f;
    }
}

}  // namespace

extern "C" int vc_noise_gain_f32(const float* d_power, const int32_t* d_n_frames, const float* d_noise0, int32_t batch,
                                 int32_t max_frames, int32_t n_bins, const vc_denoise_cfg* cfg, float* d_gain, float* d_noise,
                                 void* stream) {
    const char* fn = "vc_noise_gain_f32";
    VC_REQUIRE(d_power && d_gain && cfg, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && n_bins >= 2 && n_bins <= 2049,
               "%s: bad shape (batch %d in [1, 65535], max_frames %d >= 1, n_bins %d in [2, 2049])", fn, batch, max_frames, n_bins);
    VC_REQUIRE(cfg->rule == 0 || cfg->rule == 1, "%s: rule must be 0 (Wiener) or 1 (log-MMSE), got %d", fn, cfg->rule);
    VC_REQUIRE(cfg->n_init >= 1, "%s: n_init must be at least 1 (got %d)", fn, cfg->n_init);
    VC_REQUIRE(cfg->a_spp >= 0.0f && cfg->a_spp <= 1.0f && cfg->a_dd >= 0.0f && cfg->a_dd <= 1.0f,
               "%s: a_spp and a_dd must be in [0, 1] (got %g, %g)", fn, (double)cfg->a_spp, (double)cfg->a_dd);
    VC_REQUIRE(cfg->a_noise > 0.0f && cfg->a_noise <= 1.0f, "%s: a_noise must be in (0, 1] (got %g)", fn, (double)cfg->a_noise);
    VC_REQUIRE(std::isfinite(cfg->xi_h1) && cfg->xi_h1 > 0.0f && std::isfinite(cfg->xi_min) && cfg->xi_min > 0.0f &&
               std::isfinite(cfg->gamma_max) && cfg->gamma_max > 0.0f,
               "%s: xi_h1, xi_min and gamma_max must be finite and positive (got %g, %g, %g)", fn, (double)cfg->xi_h1,
               (double)cfg->xi_min, (double)cfg->gamma_max);
    VC_REQUIRE(cfg->gain_min > 0.0f && cfg->gain_min <= 1.0f, "%s: gain_min must be in (0, 1] (got %g)", fn, (double)cfg->gain_min);
    NgArgs a;
    a.power = d_power; a.n_frames = d_n_frames; a.noise0 = d_noise0; a.gain = d_gain; a.noise = d_noise;
    a.maxF = max_frames; a.nb = n_bins; a.cfg = *cfg;
    const dim3 grid(((unsigned)n_bins + 63) / 64, (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (cfg->rule == 1 && d_noise) hipLaunchKernelGGL((noise_gain_kernel<1, true>), grid, dim3(64), 0, st, a);
    else if (cfg->rule == 1) hipLaunchKernelGGL((noise_gain_kernel<1, false>), grid, dim3(64), 0, st, a);
    else if (d_noise) hipLaunchKernelGGL((noise_gain_kernel<0, true>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((noise_gain_kernel<0, false>), grid, dim3(64), 0, st, a);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}
