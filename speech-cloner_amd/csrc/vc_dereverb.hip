// Dereverberation (include/vc_hip.h, "Dereverberation"): weighted prediction error (WPE) in the STFT domain, one bin at a time.
//
// wpe_kernel: one workgroup per (utterance, bin).  The bin's frames come once from the contiguous bin-major row into LDS
// (float32 pairs), with the running power |y_t|^2 and the weight lam_t next to them in float64.  Per iteration:
//   lam      a lane per frame
//   R, q     the K (K + 1) / 2 upper-triangle sums and the K sums of q, ONE lane each, t ascending: the matrix is weighted,
//            hence not Toeplitz, and every entry is a serial sum over the frames.  This is the launch's time.
//   solve    complex Cholesky out of LDS, a lane per row, one column per step; the substitutions a lane per row too.  The
//            column form performs, for every row, exactly the subtractions of the row form in the same order.
//   y        a lane per frame
// y itself is never stored between iterations: only its power is read again, and the last iteration rounds y to float32
// on its way out.  Nothing is written before the last factorisation has succeeded, so a failed pivot passes x through.
//
// The whole file is compiled with contraction off: every product and every sum is rounded once, in float64.  No atomics,
// no memset, no hand-off between workgroups; fixed geometry and fixed orders.
#include <cmath>
#include "vc_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int WT = 256;
constexpr int WPE_LDS = 160 * 1024;
constexpr int MAX_TAPS = 32, MAX_DELAY = 64, MAX_ITERS = 16, MAX_CONTEXT = 8;

struct WpeArgs {
    const float* re;          // [B][nb][maxF]
    const float* im;
    const int32_t* n_frames;  // [B] or null
    float* out_re;
    float* out_im;
    float* taps;              // [B][nb][K][2] or null
    int32_t* status;          // [B][nb]
    int maxF, nb, K, D, I, c;
    float floor_rel, load_rel;
};

// R / L [K][K] complex, q / z / g [K] complex, lam0 and the flag: the bytes of LDS in front of the frames
constexpr size_t wpe_fixed_bytes(int K) { return sizeof(double) * ((size_t)2 * K * K + 2 * K + 4); }
constexpr size_t WPE_FRAME_BYTES = 2 * sizeof(double) + 2 * sizeof(float);      // p, lam, x

__global__ void __launch_bounds__(WT)
wpe_kernel(WpeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = a.K, D = a.D;
    double* Rm = reinterpret_cast<double*>(smem);      // [K][K][2]: R above and on the diagonal, then L on and below it
    double* qv = Rm + 2 * K * K;                       // [K][2]: q, then z, then g
    double* sc = qv + 2 * K;                           // lam0
    int* flag = reinterpret_cast<int*>(sc + 2);        // a pivot failed
    double* p = sc + 4;                                // [maxF]: |y_t|^2
    double* lam = p + a.maxF;                          // [maxF]
    float2* xs = reinterpret_cast<float2*>(lam + a.maxF);   // [maxF]

    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t row = ((size_t)b * a.nb + k) * a.maxF;
    const int F = a.n_frames ? min(max(a.n_frames[b], 0), a.maxF) : a.maxF;

    for (int t = tid; t < F; t += WT) {
        const float xr = a.re[row + t], xi = a.im[row + t];
        xs[t] = make_float2(xr, xi);
        p[t] = (double)xr * (double)xr + (double)xi * (double)xi;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();
    int status = F <= D ? 2 : 0;
    if (status == 0) {
        if (tid == 0) {
            double s = 0.0;
            for (int t = 0; t < F; ++t) s += p[t];
            sc[0] = (double)a.floor_rel * (s / (double)F);
        }
        __syncthreads();
        const double lam0 = sc[0];
        const int ntri = K * (K + 1) / 2, nent = ntri + K;
        for (int it = 0; it < a.I; ++it) {
            for (int t = tid; t < F; t += WT) {
                const int lo = max(t - a.c, 0), hi = min(t + a.c, F - 1);
                double s = 0.0;
                for (int u = lo; u <= hi; ++u) s += p[u];
                s = s / (double)(hi - lo + 1);
                lam[t] = s > lam0 ? s : lam0;
            }
            __syncthreads();
            // R[i][j], i <= j, and q[i]: one lane each
            for (int e = tid; e < nent; e += WT) {
                const bool isq = e >= ntri;
                int i = 0, j = 0;
                if (isq) {
                    i = e - ntri;
                } else {
                    int r = e;
                    while (r >= K - i) { r -= K - i; ++i; }
                    j = i + r;
                }
                const int oa = D + i, ob = isq ? 0 : D + j;
                double sr = 0.0, si = 0.0;
                for (int t = isq ? oa : ob; t < F; ++t) {
                    const float2 A = xs[t - oa], B = xs[t - ob];
                    const double l = lam[t];
                    const double ar = A.x, ai = A.y, br = B.x, bi = B.y;
                    const double pr = ar * br + ai * bi;          // A * conj(B)
                    const double pi = ai * br - ar * bi;
                    sr += pr / l;
                    si += pi / l;
                }
                double* dst = isq ? qv + 2 * i : Rm + 2 * (i * K + j);
                dst[0] = sr; dst[1] = si;
            }
            __syncthreads();
            if (tid == 0) {
                double tr = 0.0;
                for (int i = 0; i < K; ++i) tr += Rm[2 * (i * K + i)];
                const double add = ((double)a.load_rel * tr) / (double)K;
                for (int i = 0; i < K; ++i) Rm[2 * (i * K + i)] += add;
            }
            __syncthreads();
            // R = L L^H, column by column
            bool bad = false;
            for (int j = 0; j < K; ++j) {
                if (tid == j) {
                    double d = Rm[2 * (j * K + j)];
                    for (int m = 0; m < j; ++m) {
                        const double lr = Rm[2 * (j * K + m)], li = Rm[2 * (j * K + m) + 1];
                        d -= lr * lr + li * li;
                    }
                    if (!(d > 0.0 && d < INFINITY)) *flag = 1;
                    Rm[2 * (j * K + j)] = sqrt(d);
                }
                __syncthreads();
                bad = *flag != 0;
                if (bad) break;
                if (tid > j && tid < K) {
                    const int i = tid;
                    double sr = Rm[2 * (j * K + i)], si = -Rm[2 * (j * K + i) + 1];    // R[i][j] = conj(R[j][i])
                    for (int m = 0; m < j; ++m) {
                        const double ar = Rm[2 * (i * K + m)], ai = Rm[2 * (i * K + m) + 1];
                        const double br = Rm[2 * (j * K + m)], bi = Rm[2 * (j * K + m) + 1];
                        const double pr = ar * br + ai * bi;      // L[i][m] * conj(L[j][m])
                        const double pi = ai * br - ar * bi;
                        sr -= pr;
                        si -= pi;
                    }
                    const double dj = Rm[2 * (j * K + j)];
                    Rm[2 * (i * K + j)] = sr / dj;
                    Rm[2 * (i * K + j) + 1] = si / dj;
                }
                __syncthreads();
            }
            if (bad) { status = 1; break; }
            // L z = q, forward
            for (int m = 0; m < K; ++m) {
                if (tid == m) {
                    const double d = Rm[2 * (m * K + m)];
                    qv[2 * m] = qv[2 * m] / d;
                    qv[2 * m + 1] = qv[2 * m + 1] / d;
                }
                __syncthreads();
                if (tid > m && tid < K) {
                    const int i = tid;
                    const double ar = Rm[2 * (i * K + m)], ai = Rm[2 * (i * K + m) + 1];
                    const double zr = qv[2 * m], zi = qv[2 * m + 1];
                    const double pr = ar * zr - ai * zi;          // L[i][m] * z[m]
                    const double pi = ar * zi + ai * zr;
                    qv[2 * i] -= pr;
                    qv[2 * i + 1] -= pi;
                }
                __syncthreads();
            }
            // L^H g = z, backward
            for (int m = K - 1; m >= 0; --m) {
                if (tid == m) {
                    const double d = Rm[2 * (m * K + m)];
                    qv[2 * m] = qv[2 * m] / d;
                    qv[2 * m + 1] = qv[2 * m + 1] / d;
                }
                __syncthreads();
                if (tid < m) {
                    const int i = tid;
                    const double ar = Rm[2 * (m * K + i)], ai = Rm[2 * (m * K + i) + 1];
                    const double gr = qv[2 * m], gi = qv[2 * m + 1];
                    const double pr = ar * gr + ai * gi;          // conj(L[m][i]) * g[m]
                    const double pi = ar * gi - ai * gr;
                    qv[2 * i] -= pr;
                    qv[2 * i + 1] -= pi;
                }
                __syncthreads();
            }
            // y_t = x_t - sum_i conj(g[i]) x_{t-D-i}
            const bool last = it == a.I - 1;
            for (int t = tid; t < F; t += WT) {
                const int n = min(K, t - D + 1);
                double sr = 0.0, si = 0.0;
                for (int i = 0; i < n; ++i) {
                    const float2 U = xs[t - D - i];
                    const double gr = qv[2 * i], gi = qv[2 * i + 1], ur = U.x, ui = U.y;
                    const double pr = gr * ur + gi * ui;
                    const double pi = gr * ui - gi * ur;
                    sr += pr;
                    si += pi;
                }
                const float2 X = xs[t];
                const double yr = (double)X.x - sr, yi = (double)X.y - si;
                p[t] = yr * yr + yi * yi;
                if (last) {
                    a.out_re[row + t] = (float)yr;
                    a.out_im[row + t] = (float)yi;
                }
            }
            __syncthreads();
        }
    }
    if (status != 0)
        for (int t = tid; t < F; t += WT) {
            const float2 X = xs[t];
            a.out_re[row + t] = X.x;
            a.out_im[row + t] = X.y;
        }
    for (int t = F + tid; t < a.maxF; t += WT) {
        a.out_re[row + t] = 0.0f;
        a.out_im[row + t] = 0.0f;
    }
    if (a.taps && tid < 2 * K)
        a.taps[((size_t)b * a.nb + k) * 2 * K + tid] = status == 0 ? (float)qv[tid] : 0.0f;
    if (tid == 0) a.status[(size_t)b * a.nb + k] = status;
}

}  // namespace

extern "C" {

int32_t vc_wpe_max_frames(int32_t taps) {
    if (taps < 1 || taps > MAX_TAPS) return 0;
    return (int32_t)((WPE_LDS - wpe_fixed_bytes(taps)) / WPE_FRAME_BYTES);
}

int vc_wpe_f32(const float* d_re, const float* d_im, const int32_t* d_n_frames, int32_t batch, int32_t n_bins, int32_t max_frames,
               const vc_wpe_cfg* cfg, float* d_out_re, float* d_out_im, float* d_taps, int32_t* d_status, void* stream) {
    const char* fn = "vc_wpe_f32";
    VC_REQUIRE(d_re && d_im && cfg && d_out_re && d_out_im && d_status, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && n_bins >= 2 && n_bins <= 2049 && max_frames >= 1,
               "%s: bad shape (batch %d in [1, 65535], n_bins %d in [2, 2049], max_frames %d >= 1)", fn, batch, n_bins, max_frames);
    VC_REQUIRE(cfg->taps >= 1 && cfg->taps <= MAX_TAPS, "%s: taps must be in [1, %d] (got %d)", fn, MAX_TAPS, cfg->taps);
    VC_REQUIRE(cfg->delay >= 1 && cfg->delay <= MAX_DELAY, "%s: delay must be in [1, %d] (got %d)", fn, MAX_DELAY, cfg->delay);
    VC_REQUIRE(cfg->iterations >= 1 && cfg->iterations <= MAX_ITERS, "%s: iterations must be in [1, %d] (got %d)", fn, MAX_ITERS,
               cfg->iterations);
    VC_REQUIRE(cfg->context >= 0 && cfg->context <= MAX_CONTEXT, "%s: context must be in [0, %d] (got %d)", fn, MAX_CONTEXT,
               cfg->context);
    VC_REQUIRE(cfg->floor_rel > 0.0f && cfg->floor_rel <= 1.0f, "%s: floor_rel must be in (0, 1] (got %g)", fn, (double)cfg->floor_rel);
    VC_REQUIRE(cfg->load_rel >= 0.0f && cfg->load_rel <= 1.0f, "%s: load_rel must be in [0, 1] (got %g)", fn, (double)cfg->load_rel);
    VC_REQUIRE(max_frames <= vc_wpe_max_frames(cfg->taps), "%s: max_frames %d exceeds vc_wpe_max_frames(%d) = %d", fn, max_frames,
               cfg->taps, vc_wpe_max_frames(cfg->taps));
    if (int rc = vc::allow_dynamic_lds<wpe_kernel>(WPE_LDS)) return rc;
    WpeArgs a;
    a.re = d_re; a.im = d_im; a.n_frames = d_n_frames; a.out_re = d_out_re; a.out_im = d_out_im; a.taps = d_taps; a.status = d_status;
    a.maxF = max_frames; a.nb = n_bins; a.K = cfg->taps; a.D = cfg->delay; a.I = cfg->iterations; a.c = cfg->context;
    a.floor_rel = cfg->floor_rel; a.load_rel = cfg->load_rel;
    const size_t smem = wpe_fixed_bytes(a.K) + WPE_FRAME_BYTES * (size_t)max_frames;
    hipLaunchKernelGGL(wpe_kernel, dim3((unsigned)n_bins, (unsigned)batch), dim3(WT), smem, (hipStream_t)stream, a);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
