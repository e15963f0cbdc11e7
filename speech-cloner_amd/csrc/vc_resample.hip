// Sample-rate conversion of a ragged batch on the device (include/vc_hip.h, "Resampling"): band-limited interpolation
// with a Kaiser-windowed sinc, every phase's taps evaluated exactly on the host (no interpolated filter table).
//
//     y[m] = sum_n x[n] * g[m * down - n * up],   g[k] = h(k / up), |k| <= half,   x = 0 outside [0, len)
//
// With m * down = q * up + p (0 <= p < up) the taps of output m are g[p + j * up], j = q - n: phase p owns one row of the
// table.  Row layout: ntap4 floats (a multiple of 4, zero filled), entry t holds j = jhi - t, so that a row and the
// input samples it multiplies are both walked upwards: y[m] = sum_t row[p][t] * x[q - jhi + t].
//
// Outputs m and m + up share their phase, and q advances by exactly `down` between them.  A lane therefore keeps RO
// accumulator pairs for RO outputs of ONE phase: a tap loaded once (16-byte loads of the lane's own row, served by L1 / L2 --
// the 44.1 kHz table is 238 KB and fits no CU's LDS) feeds RO products, and the input span of the workgroup's tile
// is staged once in LDS with the zeros outside the utterance written in, so the inner loop has no bounds test.
//
// Tile: S * RO consecutive outputs, S = up * k slots (k chosen per plan so that S nearly fills whole passes of RT
// lanes).  Slot u (phase (u * down) % up) owns outputs M0 + u + i * S, i < RO; consecutive lanes write consecutive
// outputs.  Every output is one lane's chain over t = 0 .. ntap4-1 in that order, whatever the tile, the batch size
// or the other rows hold: an utterance's samples are bit-identical alone and inside any batch.
//
// Accumulation is float32 throughout, but compensated: each product's rounding error (one fmaf) and each addition's
// (Knuth's two-sum, six float32 operations, no assumption on magnitudes) are collected in a second float32 word, and
// the output is hi + lo, rounded once.  A plain float32 chain over 136 .. 405 taps leaves 2e-7 .. 1e-6 of the peak,
// which a 16 -> 48 -> 16 kHz round trip of band-limited audio shows as its whole error: the 'kaiser_best' filter itself
// returns such a signal to 2e-8.  The compensated sum is the correctly rounded float32 value in all but rare ties, at
// ten vector operations per tap instead of one.
//
// Why vector FMAs and not v_mfma_f32_32x32x2_f32: per phase the product is Toeplitz only along outputs `up` apart,
// whose inputs lie `down` apart -- for 44.1 kHz -> 16 kHz (down 441 > 374 taps) those input spans do not overlap at
// all, so a matrix form would have to materialise one gathered operand element per multiply-add in LDS first, which is
// exactly the operand traffic this form already pays, without the MFMA's layout shuffles.  Only up == 1 has the dense
// Toeplitz structure.
#include <cmath>
#include <vector>
#include "vc_common.h"

namespace {

constexpr int RT = 256;                 // lanes per workgroup
constexpr int RO = 4;                   // outputs (of one phase) per lane and slot
constexpr int MAX_SPAN = 16000;         // floats of LDS per workgroup (64,000 bytes: two workgroups per CU)
constexpr long long MAX_TABLE = 1ll << 24;      // floats (64 MB)

// (hi, lo) += x * w without losing a bit: p + e == x * w and s + err == hi + p exactly (error-free transformations).
// Contraction is off in here: fusing x * w into the addition that follows would break both identities.
__device__ __forceinline__ void add_product(float x, float w, float& hi, float& lo) {
#pragma clang fp contract(off)
    const float p = x * w;
    const float e = __builtin_fmaf(x, w, -p);
    const float s = hi + p;
    const float bb = s - hi;
    const float err = (hi - (s - bb)) + (p - bb);
    lo += err + e;
    hi = s;
}

__global__ void __launch_bounds__(RT)
resample_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int max_in, long long ld_in,
                float* __restrict__ y, int max_out, long long ld_out, const float* __restrict__ tab,
                int up, int down, int k, int ntap4, int jhi, int span) {
    extern __shared__ __align__(16) float xs[];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int S = up * k;
    const long long M0 = (long long)blockIdx.x * S * RO;           // a multiple of up
    const int len = lens ? min(max(lens[b], 0), max_in) : max_in;
    const long long len_out = min(((long long)len * up + down - 1) / down, (long long)max_out);
    const long long Mend = min(M0 + (long long)S * RO, (long long)max_out);
    float* __restrict__ yo = y + (size_t)b * ld_out;
    if (M0 >= len_out) {                                           // the zero tail: nothing to read
        for (long long m = M0 + tid; m < Mend; m += RT) yo[m] = 0.0f;
        return;
    }
    // xs[i] = x[n_min + i], zero outside the utterance; i < span = floor((S * RO - 1) * down / up) + ntap4
    const long long n_min = (M0 / up) * down - jhi;
    const float* __restrict__ xr = x + (size_t)b * ld_in;
    for (int i = tid; i < span; i += RT) {
        const long long n = n_min + i;
        xs[i] = (n >= 0 && n < len) ? xr[n] : 0.0f;
    }
    __syncthreads();
    const int step = k * down;                                     // input distance of outputs S apart
    for (int u = tid; u < S; u += RT) {
        const int p = (int)(((long long)(u % up) * down) % up);
        const int q0 = (int)(((long long)u * down) / up);          // <= floor((S - 1) * down / up)
        const float4* __restrict__ row = reinterpret_cast<const float4*>(tab + (size_t)p * ntap4);
        const float* x0 = xs + q0;                                 // last read: q0 + (RO-1) * step + ntap4 - 1 <= span - 1
        float hi[RO], lo[RO];
#pragma unroll
        for (int i = 0; i < RO; ++i) hi[i] = lo[i] = 0.0f;
        for (int t = 0; t < ntap4; t += 4) {
            const float4 w = row[t >> 2];
#pragma unroll
            for (int i = 0; i < RO; ++i) {
                const float* xi = x0 + i * step + t;
                add_product(xi[0], w.x, hi[i], lo[i]);
                add_product(xi[1], w.y, hi[i], lo[i]);
                add_product(xi[2], w.z, hi[i], lo[i]);
                add_product(xi[3], w.w, hi[i], lo[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < RO; ++i) {
            const long long m = M0 + u + (long long)i * S;
            if (m < Mend) yo[m] = m < len_out ? __fadd_rn(hi[i], lo[i]) : 0.0f;
        }
    }
}

}  // namespace

struct vc_resample_plan {
    int32_t up, down, half, jhi, ntap4, k, span;
    float* d_tab;          // [up][ntap4]
};

extern "C" {

int vc_resample_plan_create(int32_t up, int32_t down, int32_t half, const double* h_taps, vc_resample_plan** out_plan) {
    VC_REQUIRE(out_plan && h_taps, "vc_resample_plan_create: NULL argument");
    VC_REQUIRE(up > 0 && down > 0 && half >= 0, "vc_resample_plan_create: need up > 0, down > 0, half >= 0 (got %d, %d, %d)", up,
               down, half);
    // taps per phase: j from -ceil(half / up) (phase up-1 reaches furthest back) to floor(half / up)
    const long long jhi = half / up, jlo = -(((long long)half + up - 1) / up);
    const long long ntap4 = ((jhi - jlo + 1) + 3) / 4 * 4;
    if ((long long)up * ntap4 > MAX_TABLE)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_resample_plan_create: %d phases x %lld taps exceed the table limit of %lld floats",
                             up, ntap4, MAX_TABLE);
    // slots per tile S = up * k.  First among spans of at most half the LDS budget: the smallest k whose S fills >= 98 %
    // of its passes of RT lanes, else the best-filled k if that is >= 90 %.  Failing that, the same search (>= 90 %, else
    // the best-filled k) within the whole budget.
    int best_k = 0;
    double best_eff = 0.0;
    for (int pass = 0; pass < 2 && best_eff < (pass ? 0.9 : 0.98); ++pass) {
        best_k = 0; best_eff = 0.0;
        for (int k = 1; k <= RT && (long long)up * k <= 8 * RT + up; ++k) {
            const long long S = (long long)up * k;
            const long long span = ((S * RO - 1) * down) / up + ntap4;
            if (span > (pass ? MAX_SPAN : MAX_SPAN / 2)) break;
            const double eff = (double)S / (double)(((S + RT - 1) / RT) * RT);
            if (eff > best_eff + 1e-9) { best_eff = eff; best_k = k; }
            if (eff >= (pass ? 0.9 : 0.98)) break;
        }
    }
    if (best_k == 0)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_resample_plan_create: ratio %d/%d with %lld taps per phase needs more than %d "
                             "input samples in LDS per tile", up, down, ntap4, MAX_SPAN);
    std::vector<float> tab((size_t)up * ntap4, 0.0f);
    for (int p = 0; p < up; ++p)
        for (long long t = 0; t < ntap4; ++t) {
            const long long kk = p + (jhi - t) * up;
            if (kk >= -(long long)half && kk <= half) tab[(size_t)p * ntap4 + t] = (float)h_taps[kk + half];
        }
    vc_resample_plan* pl = new vc_resample_plan();
    pl->up = up; pl->down = down; pl->half = half; pl->jhi = (int32_t)jhi; pl->ntap4 = (int32_t)ntap4; pl->k = best_k;
    pl->span = (int32_t)((((long long)up * best_k * RO - 1) * down) / up + ntap4);
    pl->d_tab = nullptr;
    if (hipMalloc(&pl->d_tab, tab.size() * sizeof(float)) != hipSuccess) {
        delete pl;
        return vc::set_error(VC_ERR_HIP, "vc_resample_plan_create: hipMalloc failed");
    }
    if (hipMemcpy(pl->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(pl->d_tab); delete pl;
        return vc::set_error(VC_ERR_HIP, "vc_resample_plan_create: hipMemcpy failed");
    }
    *out_plan = pl;
    return VC_OK;
}

void vc_resample_plan_destroy(vc_resample_plan* plan) {
    if (!plan) return;
    if (plan->d_tab) (void)hipFree(plan->d_tab);
    delete plan;
}

int vc_resample_f32(const vc_resample_plan* plan, const float* d_in, const int32_t* d_lens_in, int32_t batch, int32_t max_in,
                    int32_t ld_in, float* d_out, int32_t max_out, int32_t ld_out, void* stream) {
    VC_REQUIRE(plan && d_in && d_out, "vc_resample_f32: NULL argument");
    VC_REQUIRE(batch > 0 && batch <= 65535 && max_in > 0 && ld_in >= max_in && max_out > 0 && ld_out >= max_out,
               "vc_resample_f32: bad shape (batch %d, max_in %d, ld_in %d, max_out %d, ld_out %d)", batch, max_in, ld_in, max_out, ld_out);
    const long long need = ((long long)max_in * plan->up + plan->down - 1) / plan->down;
    VC_REQUIRE(max_out >= need, "vc_resample_f32: max_out %d < ceil(max_in * up / down) = %lld", max_out, need);
    const long long tile = (long long)plan->up * plan->k * RO;
    const dim3 grid((unsigned)((max_out + tile - 1) / tile), batch);
    hipLaunchKernelGGL(resample_kernel, grid, dim3(RT), (size_t)plan->span * sizeof(float), (hipStream_t)stream, d_in, d_lens_in,
                       max_in, (long long)ld_in, d_out, max_out, (long long)ld_out, plan->d_tab, plan->up, plan->down, plan->k,
                       plan->ntap4, plan->jhi, plan->span);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
