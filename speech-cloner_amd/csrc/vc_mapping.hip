// Spectral mapping on the device (include/vc_hip.h, "Spectral mapping"): the joint-density Gaussian mixture of Toda, Black and
// Tokuda (2007) over pairs of source and target feature vectors -- every dimension of every component carries a 2 x 2
// covariance --, its EM, the conversion statistics of a source utterance, maximum-likelihood parameter generation (MLPG) and the
// gain that turns converted cepstra into a differential filter.
//
// jd_prepare_kernel: the table the other kernels read, elementwise, float64, each output rounded once.  Six arrays
// TRANSPOSED to [d][m] (lane m of a wave reads consecutive words for every d): mu_x, mu_y, a, b, g, 1 / sxx; c [M], cx [M];
// and four arrays [m][d] (lane d reads consecutive words for every m): mu_x, mu_y, A, 1 / Dv.
//
// jd_accumulate_kernel: the E-step over the cells of a DTW path without the posterior matrix.  Grid = (chunks of 64
// components) x (128 partitions): constants and arguments.  Tile k (32 cells) of pair b goes to partition (b + k) % 128; a
// workgroup of 512 lanes walks its pairs and tiles ascending.  Per tile: the joint vectors are gathered through the path
// into LDS; lane t forms l_m of component t % M' for four cells at a time into LDS [cell][m] (all M components: ll needs
// them; with more than one chunk this part is repeated per chunk); one wave per cell forms ll as vc_gmm_loglik_f32 does;
// gamma of the chunk's components goes to LDS [cell][64]; then lane (m = t & 63, r = t >> 6) adds, cell by cell, the five
// products of the dimensions d = r, r + 8, ... into float64 REGISTERS: at most 8 dimensions, 40 accumulators and N -- 82
// VGPRs of accumulators at 512 lanes, where the speaker kernel's split over four lane groups would need 162.
// jd_reduce_kernel adds the partitions of an element in the order 0 .. 127.
//
// jd_update_kernel: elementwise over (component, dimension), float64, each output rounded once.
//
// jd_map_kernel: one workgroup of 256 lanes per (utterance, tile of 32 frames): lane m forms l_m of the marginal x-mixture
// for eight frames at a time; one wave per frame forms ll, the arg-max and (soft) gamma in place; then lane (d = t & 63,
// r = t >> 6) sums over the components ascending for the frames r, r + 4, ...
//
// mlpg_kernel: one wave per utterance, lane j = static dimension j.  Banded LDL^T in float64 by rows, the last four rows of
// the factor in registers.  The chain of a row is a few dozen dependent float64 operations; what a row reads from memory
// does not depend on the chain, so it is loaded three rows ahead into a register window (the inputs going forward, the
// factor going back) and the chain never waits for a load.  The factor goes to the workspace by columns,
// [utterance][i][5][n] = L[i + 4 .. i + 1, i] and u_i = z_i / d_i: the lanes of the wave write and read consecutive words
// and the back substitution reads one row per step, descending.
//
// cep_gain_kernel: one workgroup per (utterance, tile of 8 frames): the cepstral difference to LDS, its inverse DCT to LDS
// [frame][band], then one lane per (frame, bin).
//
// The whole file is compiled with contraction off; a fused multiply-add is written fma / fmaf where the definition has
// one.  No atomics, no memset, no hand-off between workgroups; fixed geometry and fixed orders.
#include <cmath>
#include "vc_device.h"

#pragma clang fp contract(off)

#ifndef VC_MLPG_REAL
#define VC_MLPG_REAL double
#endif

namespace {

constexpr int MAX_M = 256;
constexpr int MAX_D = 64;
constexpr int MAX_CEP = 32;
constexpr int MAX_ELEMS = 1 << 30;      // frames * D of one utterance
constexpr int MAX_PATH = 1 << 24;       // cells of one pair
constexpr int TILE = 32;                // cells (accumulate) or frames (map) per tile
constexpr int CHUNK = 64;               // components per accumulate workgroup
constexpr int PARTS = 128;              // partitions of the cells
constexpr int ACC_NT = 512;
constexpr int ACC_R = ACC_NT / CHUNK;   // lane groups of the accumulate kernel: 8
constexpr int DQ = MAX_D / ACC_R;       // dimensions per lane: 8
constexpr int MAP_NT = 256;
constexpr int NT = 256;
constexpr int GAIN_TILE = 8;
constexpr int GAIN_MAX_MELS = 128;
constexpr int GAIN_MAX_BINS = 2049;
constexpr int MLPG_MAX_F = 1 << 20;

__host__ __device__ inline size_t blk_doubles(int D) { return (size_t)CHUNK * (1 + 5 * D) + 2; }
__host__ __device__ inline size_t table_floats(int M, int D) { return (size_t)10 * M * D + 2 * (size_t)M; }
inline unsigned blocks_for(size_t n) { return (unsigned)((n + NT - 1) / NT); }

struct JdTable {
    const float *mxT, *myT, *aT, *bT, *gT, *ivxT, *c, *cx, *mx, *my, *A, *iDv;
};
__host__ __device__ inline JdTable split_table(const float* t, int M, int D) {
    const size_t n = (size_t)M * D;
    JdTable r;
    r.mxT = t; r.myT = t + n; r.aT = t + 2 * n; r.bT = t + 3 * n; r.gT = t + 4 * n; r.ivxT = t + 5 * n;
    r.c = t + 6 * n; r.cx = r.c + M;
    r.mx = r.cx + M; r.my = r.mx + n; r.A = r.my + n; r.iDv = r.A + n;
    return r;
}

// ------------------------------------------------------------------------------------------------------------- prepare
__global__ void __launch_bounds__(NT)
jd_prepare_kernel(const float* __restrict__ w, const float* __restrict__ mu_x, const float* __restrict__ mu_y,
                  const float* __restrict__ var_x, const float* __restrict__ var_y, const float* __restrict__ cov, int M, int D,
                  float* __restrict__ table) {
    const size_t n = (size_t)M * D;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= table_floats(M, D)) return;
    if (i < 6 * n) {                                                // transposed arrays: i = which * n + d * M + m
        const int which = (int)(i / n);
        const size_t j = i % n;
        const int m = (int)(j % M), d = (int)(j / M);
        const size_t s = (size_t)m * D + d;
        const double sxx = (double)var_x[s], syy = (double)var_y[s], sxy = (double)cov[s];
        const double det = sxx * syy - sxy * sxy;
        float v;
        switch (which) {
            case 0: v = mu_x[s]; break;
            case 1: v = mu_y[s]; break;
            case 2: v = (float)(syy / det); break;
            case 3: v = (float)(sxy / det); break;
            case 4: v = (float)(sxx / det); break;
            default: v = (float)(1.0 / sxx); break;
        }
        table[i] = v;
    } else if (i < 6 * n + 2 * (size_t)M) {
        const size_t j = i - 6 * n;
        const int m = (int)(j % M);
        const bool joint = j < (size_t)M;
        double acc = 0.0;
        for (int d = 0; d < D; ++d) {
            const size_t s = (size_t)m * D + d;
            const double sxx = (double)var_x[s], syy = (double)var_y[s], sxy = (double)cov[s];
            if (joint) {
                const double det = sxx * syy - sxy * sxy;
                acc = acc + log(39.478417604357434475 * det);      // (2 pi)^2
            } else {
                acc = acc + log(6.283185307179586476925 * sxx);
            }
        }
        table[i] = (float)(log((double)w[m]) - 0.5 * acc);
    } else {                                                        // row-major arrays: i = base + which * n + m * D + d
        const size_t j = i - 6 * n - 2 * (size_t)M;
        const int which = (int)(j / n);
        const size_t s = j % n;
        const double sxx = (double)var_x[s], syy = (double)var_y[s], sxy = (double)cov[s];
        float v;
        switch (which) {
            case 0: v = mu_x[s]; break;
            case 1: v = mu_y[s]; break;
            case 2: v = (float)(sxy / sxx); break;
            default: v = (float)(1.0 / (syy - sxy * sxy / sxx)); break;
        }
        table[i] = v;
    }
}

// ll of one cell or frame from its l_m in LDS (row of MAX_M floats): lane l of the wave takes components l, l + 64, ...
// ascending, maximum and sum by butterflies; best = the smallest m that attains the maximum
__device__ inline float wave_logsumexp(const float* __restrict__ row, int M, int lane, int* best) {
    float v[MAX_M / 64];
    float mx = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < MAX_M / 64; ++k) {
        v[k] = lane + 64 * k < M ? row[lane + 64 * k] : -__builtin_inff();
        mx = fmaxf(mx, v[k]);
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sh, 64));
    float sum = 0.0f;
    int arg = MAX_M;
#pragma unroll
    for (int k = MAX_M / 64 - 1; k >= 0; --k)
        if (lane + 64 * k < M && v[k] == mx) arg = lane + 64 * k;
#pragma unroll
    for (int k = 0; k < MAX_M / 64; ++k)
        if (lane + 64 * k < M) sum += expf(v[k] - mx);
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        sum += __shfl_xor(sum, sh, 64);
        arg = min(arg, __shfl_xor(arg, sh, 64));
    }
    if (best) *best = arg;
    return mx + logf(sum);
}

// ---------------------------------------------------------------------------------------------------------- accumulate
// partial block of a workgroup: [CHUNK] N, five times [CHUNK][D] (Sx, Sy, Sxx, Syy, Sxy), L, count
__global__ void __launch_bounds__(ACC_NT)
jd_accumulate_kernel(const float* __restrict__ fa, const float* __restrict__ fb, const int32_t* __restrict__ len_a,
                     const int32_t* __restrict__ len_b, const int32_t* __restrict__ path, const int32_t* __restrict__ path_len,
                     int batch, int Fa, int Fb, int max_path, int D, const float* __restrict__ table, int M,
                     double* __restrict__ ws) {
    __shared__ float xs[TILE * MAX_D];
    __shared__ float ys[TILE * MAX_D];
    __shared__ float lbuf[TILE * MAX_M];
    __shared__ float gam[TILE * CHUNK];
    __shared__ float lls[TILE];
    __shared__ int ci[TILE], cj[TILE];
    const int c = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const int ml = t & 63, r = t >> 6;
    const size_t MD = (size_t)M * D;                                // table: mu_x, mu_y, a, b, g transposed, MD floats each
    double sx[DQ], sy[DQ], sxx[DQ], syy[DQ], sxy[DQ];
#pragma unroll
    for (int j = 0; j < DQ; ++j) sx[j] = sy[j] = sxx[j] = syy[j] = sxy[j] = 0.0;
    double nsum = 0.0, lsum = 0.0, cnt = 0.0;
    for (int b = 0; b < batch; ++b) {                               // uniform over the workgroup
        const int la = min(max(len_a[b], 0), Fa), lb = min(max(len_b[b], 0), Fb);
        const int n_cells = path ? min(max(path_len[b], 0), max_path) : min(la, lb);
        const int n_tiles = (n_cells + TILE - 1) / TILE;
        const float* __restrict__ XA = fa + (size_t)b * Fa * D;
        const float* __restrict__ XB = fb + (size_t)b * Fb * D;
        for (int k = (p - b % PARTS + PARTS) % PARTS; k < n_tiles; k += PARTS) {
            const int p0 = k * TILE;
            __syncthreads();                                        // the previous tile's reads
            if (t < TILE) {
                int i = -1, j = -1;
                if (p0 + t < n_cells) {
                    if (path) {
                        i = path[((size_t)b * max_path + p0 + t) * 2];
                        j = path[((size_t)b * max_path + p0 + t) * 2 + 1];
                    } else {
                        i = j = p0 + t;
                    }
                }
                const bool ok = i >= 0 && i < la && j >= 0 && j < lb;
                ci[t] = ok ? i : -1;
                cj[t] = ok ? j : -1;
            }
            __syncthreads();
            for (int e = t; e < TILE * D; e += ACC_NT) {
                const int f = e / D, d = e - f * D;
                const bool ok = ci[f] >= 0;
                xs[e] = ok ? XA[(size_t)ci[f] * D + d] : 0.0f;
                ys[e] = ok ? XB[(size_t)cj[f] * D + d] : 0.0f;
            }
            __syncthreads();
            for (int e = t; e < (TILE / 4) * M; e += ACC_NT) {      // l_m of four cells: component e % M, cells 4 (e / M) ..
                const int mm = e % M, f0 = 4 * (e / M);
                float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int d = 0; d < D; ++d) {
                    const float* __restrict__ tb = table + (size_t)d * M + mm;
                    const float mx = tb[0], my = tb[MD], av = tb[2 * MD], bv = tb[3 * MD], gv = tb[4 * MD];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float dx = xs[(f0 + j) * D + d] - mx, dy = ys[(f0 + j) * D + d] - my;
                        q[j] = fmaf(av * dx, dx, q[j]);
                        q[j] = fmaf(-2.0f * bv * dx, dy, q[j]);
                        q[j] = fmaf(gv * dy, dy, q[j]);
                    }
                }
                const float cm = table[6 * MD + mm];
#pragma unroll
                for (int j = 0; j < 4; ++j) lbuf[(f0 + j) * MAX_M + mm] = fmaf(-0.5f, q[j], cm);
            }
            __syncthreads();
            for (int f = r; f < TILE; f += ACC_R) {                 // uniform over the wave
                const float v = ci[f] >= 0 ? wave_logsumexp(lbuf + f * MAX_M, M, ml, nullptr) : 0.0f;
                if (ml == 0) lls[f] = v;
            }
            __syncthreads();
            for (int e = t; e < TILE * CHUNK; e += ACC_NT) {
                const int f = e / CHUNK, k2 = e - f * CHUNK, mm = c * CHUNK + k2;
                gam[e] = mm < M && ci[f] >= 0 ? expf(lbuf[f * MAX_M + mm] - lls[f]) : 0.0f;
            }
            __syncthreads();
            for (int f = 0; f < TILE; ++f) {
                if (ci[f] < 0) continue;                            // uniform over the workgroup
                const double gm = (double)gam[f * CHUNK + ml];
                if (r == 0) nsum += gm;
#pragma unroll
                for (int j = 0; j < DQ; ++j) {                      // (a lane beyond D adds column D - 1 again and stores nothing)
                    const int d = min(r + ACC_R * j, D - 1);
                    const double xv = (double)xs[f * D + d], yv = (double)ys[f * D + d];
                    const double gx = gm * xv, gy = gm * yv;
                    sx[j] += gx;
                    sy[j] += gy;
                    sxx[j] = fma(gx, xv, sxx[j]);
                    syy[j] = fma(gy, yv, syy[j]);
                    sxy[j] = fma(gx, yv, sxy[j]);
                }
                if (t == 0) {
                    lsum += (double)lls[f];
                    cnt += 1.0;
                }
            }
        }
    }
    double* blk = ws + ((size_t)p * gridDim.x + c) * blk_doubles(D);
    const size_t CD = (size_t)CHUNK * D;
    if (r == 0) blk[ml] = nsum;
#pragma unroll
    for (int j = 0; j < DQ; ++j) {
        const int d = r + ACC_R * j;
        if (d < D) {
            double* q = blk + CHUNK + (size_t)ml * D + d;
            q[0] = sx[j];
            q[CD] = sy[j];
            q[2 * CD] = sxx[j];
            q[3 * CD] = syy[j];
            q[4 * CD] = sxy[j];
        }
    }
    if (t == 0) {
        blk[CHUNK + 5 * CD] = lsum;
        blk[CHUNK + 5 * CD + 1] = cnt;
    }
}

// out element e: e < M: N; then five blocks of M D; then L, count
__global__ void __launch_bounds__(NT)
jd_reduce_kernel(const double* __restrict__ ws, int M, int D, int chunks, double* __restrict__ outN, double* __restrict__ outS,
                 double* __restrict__ outL) {
    const size_t MD = (size_t)M * D, CD = (size_t)CHUNK * D;
    const size_t per = (size_t)M + 5 * MD + 2;
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= per) return;
    int m = 0;
    size_t off;
    double* dst;
    if (e < (size_t)M) {
        m = (int)e;
        off = m % CHUNK;
        dst = outN + m;
    } else if (e < M + 5 * MD) {
        const size_t j = e - M;
        const size_t which = j / MD, jj = j % MD;
        m = (int)(jj / D);
        off = CHUNK + which * CD + (size_t)(m % CHUNK) * D + jj % D;
        dst = outS + j;
    } else {
        off = CHUNK + 5 * CD + (e - M - 5 * MD);
        dst = outL + (e - M - 5 * MD);
    }
    const int c = m / CHUNK;
    double acc = 0.0;
    for (int p = 0; p < PARTS; ++p) acc += ws[((size_t)p * chunks + c) * blk_doubles(D) + off];
    *dst = acc;
}

// -------------------------------------------------------------------------------------------------------------- update
__global__ void __launch_bounds__(NT)
jd_update_kernel(const double* __restrict__ N, const double* __restrict__ S, int M, int D, const float* __restrict__ mx_in,
                 const float* __restrict__ my_in, const float* __restrict__ vx_in, const float* __restrict__ vy_in,
                 const float* __restrict__ cov_in, const float* __restrict__ floor_x, const float* __restrict__ floor_y,
                 float rho_max, float min_count, float* __restrict__ w_out, float* __restrict__ mx_out, float* __restrict__ my_out,
                 float* __restrict__ vx_out, float* __restrict__ vy_out, float* __restrict__ cov_out) {
    const size_t MD = (size_t)M * D;
    const size_t j = (size_t)blockIdx.x * NT + threadIdx.x;
    if (j >= MD) return;
    const int m = (int)(j / D), d = (int)(j % D);
    const double n = N[m];
    if (d == 0) {
        double tot = 0.0;
        for (int k = 0; k < M; ++k) tot += N[k];
        const double wv = n / tot;
        w_out[m] = (float)(wv > 0x1p-40 ? wv : 0x1p-40);
    }
    if (!(n >= (double)min_count) || !(n > 0.0)) {
        mx_out[j] = mx_in[j];
        my_out[j] = my_in[j];
        vx_out[j] = vx_in[j];
        vy_out[j] = vy_in[j];
        cov_out[j] = cov_in[j];
        return;
    }
    const double ux = S[j] / n, uy = S[MD + j] / n;
    const double rx = S[2 * MD + j] / n - ux * ux, ry = S[3 * MD + j] / n - uy * uy;
    const double fx = (double)floor_x[d], fy = (double)floor_y[d];
    const double vx = rx > fx ? rx : fx, vy = ry > fy ? ry : fy;
    const double lim = (double)rho_max * sqrt(vx * vy);
    double cv = S[4 * MD + j] / n - ux * uy;
    cv = cv > lim ? lim : cv;
    cv = cv < -lim ? -lim : cv;
    mx_out[j] = (float)ux;
    my_out[j] = (float)uy;
    vx_out[j] = (float)vx;
    vy_out[j] = (float)vy;
    cov_out[j] = (float)cv;
}

// ----------------------------------------------------------------------------------------------------------------- map
__global__ void __launch_bounds__(MAP_NT)
jd_map_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int max_frames, int D, const float* __restrict__ table,
              int M, int mixture, float* __restrict__ outP, float* __restrict__ outR, float* __restrict__ outE,
              int32_t* __restrict__ outBest) {
    __shared__ float xs[TILE * MAX_D];
    __shared__ float lbuf[TILE * MAX_M];
    __shared__ int bests[TILE];
    const int b = blockIdx.y, f0 = blockIdx.x * TILE, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int len = min(max(lens[b], 0), max_frames);
    const int nf = min(TILE, len - f0);                             // frames of this tile below len
    const int n_out = min(TILE, max_frames - f0);
    const size_t row0 = (size_t)b * max_frames + f0;
    if (nf <= 0) {
        for (int e = t; e < n_out * D; e += MAP_NT) {
            outP[row0 * D + e] = 0.0f;
            outR[row0 * D + e] = 0.0f;
            if (outE) outE[row0 * D + e] = 0.0f;
        }
        if (outBest && t < n_out) outBest[row0 + t] = 0;
        return;
    }
    const JdTable T = split_table(table, M, D);
    for (int i = t; i < TILE * D; i += MAP_NT) xs[i] = i < nf * D ? x[row0 * D + i] : 0.0f;
    __syncthreads();
    if (t < M) {
        const float cm = T.cx[t];
        for (int g0 = 0; g0 < nf; g0 += 8) {
            float q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = 0.0f;
            for (int d = 0; d < D; ++d) {
                const float mu = T.mxT[(size_t)d * M + t], iv = T.ivxT[(size_t)d * M + t];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float df = xs[(g0 + j) * D + d] - mu;
                    q[j] = fmaf(df * df, iv, q[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) lbuf[(g0 + j) * MAX_M + t] = fmaf(-0.5f, q[j], cm);
        }
    }
    __syncthreads();
    for (int f = wave; f < nf; f += MAP_NT / 64) {                  // uniform over the wave; gamma replaces l_m in place
        int best;
        const float ll = wave_logsumexp(lbuf + f * MAX_M, M, lane, &best);
        for (int k = lane; k < M; k += 64) lbuf[f * MAX_M + k] = expf(lbuf[f * MAX_M + k] - ll);
        if (lane == 0) bests[f] = best;
    }
    __syncthreads();
    if (outBest && t < n_out) outBest[row0 + t] = t < nf ? bests[t] : 0;
    if (lane < D) {
        const int d = lane;
        for (int f = wave; f < n_out; f += MAP_NT / 64) {
            float P = 0.0f, R = 0.0f, E = 0.0f;
            if (f < nf) {
                const float xv = xs[f * D + d];
                const int lo = mixture ? bests[f] : 0, hi = mixture ? bests[f] + 1 : M;
                for (int m = lo; m < hi; ++m) {
                    const size_t o = (size_t)m * D + d;
                    const float gmm = mixture ? 1.0f : lbuf[f * MAX_M + m];
                    const float e = fmaf(T.A[o], xv - T.mx[o], T.my[o]);
                    const float gp = gmm * T.iDv[o];
                    P = P + gp;
                    R = fmaf(gp, e, R);
                    E = fmaf(gmm, e, E);
                }
            }
            outP[(row0 + f) * D + d] = P;
            outR[(row0 + f) * D + d] = R;
            if (outE) outE[(row0 + f) * D + d] = E;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- mlpg
// the integer weight (times 1/10) of y_i in the delta of frame t of an utterance of F frames: indices clamped as
// vc_spk_features_f32 clamps them
__device__ inline int delta_weight(int t, int i, int F) {
    const int p1 = min(t + 1, F - 1), m1 = max(t - 1, 0), p2 = min(t + 2, F - 1), m2 = max(t - 2, 0);
    return (i == p1) - (i == m1) + 2 * ((i == p2) - (i == m2));
}

// the same weight where no index is clamped (2 <= t <= F - 3): a function of the offset o = i - t alone
__device__ constexpr int interior_weight(int o) { return o == 1 ? 1 : o == -1 ? -1 : o == 2 ? 2 : o == -2 ? -2 : 0; }

constexpr int MLPG_PF = 3;              // rows loaded ahead of the row being eliminated
constexpr int MLPG_NW = 5 + MLPG_PF;    // window: entry q holds frame i - 2 + q

// Row i of the system from the windows (entry q: frame t = i - 2 + q): A[i, i - 4 + s] for s = 0 .. 4 and b_i.  Terms whose
// integer weight is 0 are left out; the others are added with t ascending.  INTERIOR: no index of the five frames is
// clamped, the weights are constants and the zero terms fall out at compile time.
template <typename real, bool INTERIOR>
__device__ __forceinline__ void mlpg_row(int i, int F, const float (&wpd)[MLPG_NW], const float (&wrd)[MLPG_NW], float ps, float rs,
                                         real (&arow)[5], real& bi) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        real acc = (real)0;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int t = i - 2 + q, k = i - 4 + s;
            const int w = INTERIOR ? interior_weight(2 - q) * interior_weight(s - q - 2)
                                   : (t >= 0 && t < F && k >= 0 ? delta_weight(t, i, F) * delta_weight(t, k, F) : 0);
            if (w != 0) acc = acc + (real)w * (real)wpd[q];
        }
        arow[s] = acc / (real)100;
    }
    arow[4] = (real)ps + arow[4];
    real racc = (real)0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int t = i - 2 + q;
        const int w = INTERIOR ? interior_weight(2 - q) : (t >= 0 && t < F ? delta_weight(t, i, F) : 0);
        if (w != 0) racc = racc + (real)w * (real)wrd[q];
    }
    bi = (real)rs + racc / (real)10;
}

template <typename real>
__global__ void __launch_bounds__(64)
mlpg_kernel(const float* __restrict__ P, const float* __restrict__ R, const int32_t* __restrict__ lens, int max_frames, int n,
            float* __restrict__ y, int32_t* __restrict__ flags, real* __restrict__ ws) {
    const int b = blockIdx.x, j = threadIdx.x;
    const int F = min(max(lens[b], 0), max_frames);
    const int D = 2 * n;
    const bool live = j < n;
    const float* __restrict__ Pb = P + (size_t)b * max_frames * D;
    const float* __restrict__ Rb = R + (size_t)b * max_frames * D;
    float* __restrict__ yb = y + (size_t)b * max_frames * n;
    // workspace row i: L[i + 4, i], L[i + 3, i], L[i + 2, i], L[i + 1, i] (column i of the factor, what the back substitution
    // of row i reads) and u_i; entries of rows beyond F - 1 are never written and never used
    real* __restrict__ W = ws + (size_t)b * max_frames * 5 * n;
    bool bad = false;
    if (live) {
        // Lr[q][s] = L[i - 1 - q, i - 5 - q + s] (row i - 1 - q of the factor, its four entries left of the diagonal);
        // dg[q] = d_{i - 1 - q}; zz[q] = z_{i - 1 - q}.  Rows before the first are 0 with d = 1.
        real Lr[4][4], dg[4], zz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            dg[q] = (real)1;
            zz[q] = (real)0;
#pragma unroll
            for (int s = 0; s < 4; ++s) Lr[q][s] = (real)0;
        }
        // the inputs of frames i - 2 .. i + 2 + MLPG_PF, loaded MLPG_PF rows ahead of their first use (0 outside the utterance)
        float wpd[MLPG_NW], wrd[MLPG_NW], wps[MLPG_NW], wrs[MLPG_NW];
        wpd[0] = wrd[0] = wps[0] = wrs[0] = 0.0f;
#pragma unroll
        for (int q = 1; q < MLPG_NW; ++q) {
            const int t = q - 3;
            const bool in = t >= 0 && t < F;
            wps[q] = in ? Pb[(size_t)t * D + j] : 0.0f;
            wpd[q] = in ? Pb[(size_t)t * D + n + j] : 0.0f;
            wrs[q] = in ? Rb[(size_t)t * D + j] : 0.0f;
            wrd[q] = in ? Rb[(size_t)t * D + n + j] : 0.0f;
        }
        for (int i = 0; i < F; ++i) {
#pragma unroll
            for (int q = 0; q < MLPG_NW - 1; ++q) {
                wps[q] = wps[q + 1];
                wpd[q] = wpd[q + 1];
                wrs[q] = wrs[q + 1];
                wrd[q] = wrd[q + 1];
            }
            {
                const int t = i + 2 + MLPG_PF;
                const bool in = t < F;
                wps[MLPG_NW - 1] = in ? Pb[(size_t)t * D + j] : 0.0f;
                wpd[MLPG_NW - 1] = in ? Pb[(size_t)t * D + n + j] : 0.0f;
                wrs[MLPG_NW - 1] = in ? Rb[(size_t)t * D + j] : 0.0f;
                wrd[MLPG_NW - 1] = in ? Rb[(size_t)t * D + n + j] : 0.0f;
            }
            real arow[5], bi;
            if (i >= 4 && i + 5 <= F) mlpg_row<real, true>(i, F, wpd, wrd, wps[2], wrs[2], arow, bi);      // uniform over the wave
            else mlpg_row<real, false>(i, F, wpd, wrd, wps[2], wrs[2], arow, bi);
            // v_s = A[i, k] - sum_{p < k} v_p L[k, p], k = i - 4 + s ascending; L[i, k] = v_s / d_k
            real v[4], Li[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                real acc = arow[s];
                // row k = i - 4 + s is Lr[3 - s]; its entry for column p = i - 4 + u (u < s) is Lr[3 - s][u + 4 - s]
#pragma unroll
                for (int u = 0; u < s; ++u) acc = acc - v[u] * Lr[3 - s][u + 4 - s];
                v[s] = acc;
                Li[s] = acc / dg[3 - s];
            }
            real di = arow[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) di = di - v[s] * Li[s];
            real zi = bi;
#pragma unroll
            for (int s = 0; s < 4; ++s) zi = zi - Li[s] * zz[3 - s];
            if (!(di > (real)0) || !(di < (real)__builtin_inf())) bad = true;
#pragma unroll
            for (int s = 0; s < 4; ++s)                              // L[i, i - 4 + s] goes to row i - 4 + s, slot s
                if (i - 4 + s >= 0) W[((size_t)(i - 4 + s) * 5 + s) * n + j] = Li[s];
            W[((size_t)i * 5 + 4) * n + j] = zi / di;
#pragma unroll
            for (int q = 3; q > 0; --q) {
                dg[q] = dg[q - 1];
                zz[q] = zz[q - 1];
#pragma unroll
                for (int s = 0; s < 4; ++s) Lr[q][s] = Lr[q - 1][s];
            }
            dg[0] = di;
            zz[0] = zi;
#pragma unroll
            for (int s = 0; s < 4; ++s) Lr[0][s] = Li[s];
        }
    }
    const bool any_bad = __ballot(bad) != 0;
    if (j == 0) flags[b] = any_bad ? 1 : 0;
    if (!live) return;
    if (bad) {
        for (int i = 0; i < F; ++i) yb[(size_t)i * n + j] = (float)((real)Rb[(size_t)i * D + j] / (real)Pb[(size_t)i * D + j]);
    } else {
        // y_i = u_i - sum_{k = i + 1 .. i + 4} L[k, i] y_k, k ascending; yy[q] = y_{i + 1 + q}.  ring[r]: workspace row i - r,
        // loaded MLPG_PF rows before its use; slot 3 - q of row i holds L[i + 1 + q, i]
        real yy[4] = {(real)0, (real)0, (real)0, (real)0};
        real ring[MLPG_PF + 1][5];
#pragma unroll
        for (int r = 0; r < MLPG_PF; ++r)
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int row = F - 1 - r;
                ring[r + 1][s] = row >= 0 ? W[((size_t)row * 5 + s) * n + j] : (real)0;
            }
        for (int i = F - 1; i >= 0; --i) {
#pragma unroll
            for (int r = 0; r < MLPG_PF; ++r)
#pragma unroll
                for (int s = 0; s < 5; ++s) ring[r][s] = ring[r + 1][s];
#pragma unroll
            for (int s = 0; s < 5; ++s) ring[MLPG_PF][s] = i - MLPG_PF >= 0 ? W[((size_t)(i - MLPG_PF) * 5 + s) * n + j] : (real)0;
            real acc = ring[0][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const real l = i + 1 + q < F ? ring[0][3 - q] : (real)0;
                acc = acc - l * yy[q];
            }
            yb[(size_t)i * n + j] = (float)acc;
            yy[3] = yy[2];
            yy[2] = yy[1];
            yy[1] = yy[0];
            yy[0] = acc;
        }
    }
    for (int i = F; i < max_frames; ++i) yb[(size_t)i * n + j] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------- gain
__global__ void __launch_bounds__(NT)
cep_gain_kernel(const float* __restrict__ cy, const float* __restrict__ cx, const int32_t* __restrict__ n_frames, int maxF, int n,
                const float* __restrict__ dct, int n_mels, const int32_t* __restrict__ bin_i0, const float* __restrict__ bin_w, int nb,
                float alpha, float db_scale, float boost, float cut, float* __restrict__ gain) {
    __shared__ float df[GAIN_TILE * MAX_CEP];
    __shared__ float dm[GAIN_TILE * GAIN_MAX_MELS];
    const int b = blockIdx.y, f0 = blockIdx.x * GAIN_TILE, t = threadIdx.x;
    const int F = n_frames ? min(max(n_frames[b], 0), maxF) : maxF;
    const int rows = min(GAIN_TILE, maxF - f0);
    const int live = min(max(F - f0, 0), rows);
    const size_t base = (size_t)b * maxF + f0;
    for (int e = t; e < live * n; e += NT) df[e] = cy[base * n + e] - cx[base * n + e];
    __syncthreads();
    for (int e = t; e < live * n_mels; e += NT) {
        const int f = e / n_mels, k = e - f * n_mels;
        float acc = 0.0f;
        for (int i = 0; i < n; ++i) {
            const float m = dct[(size_t)i * n_mels + k] * df[f * n + i];
            acc = acc + m;
        }
        dm[f * GAIN_MAX_MELS + k] = acc;
    }
    __syncthreads();
    const float sc = alpha * db_scale;
    for (int e = t; e < rows * nb; e += NT) {
        const int f = e / nb, k = e - f * nb;
        float G = 0.0f;
        if (f < live) {
            const int i0 = min(max(bin_i0[k], 0), n_mels - 2);
            const float w = bin_w[k];
            const float lo = (1.0f - w) * dm[f * GAIN_MAX_MELS + i0], hi = w * dm[f * GAIN_MAX_MELS + i0 + 1];
            const float s = fminf(fmaxf(sc * (lo + hi), -cut), boost);
            G = exp2f(s * 0.16609640474436813f);                    // float32(log2(10) / 20)
        }
        gain[base * nb + e] = G;
    }
}

inline bool shape_ok(int M, int D) { return M >= 1 && M <= MAX_M && D >= 1 && D <= MAX_D; }
inline bool frames_ok(int batch, int max_frames, int D) { return batch <= 65535 && (int64_t)max_frames * D <= MAX_ELEMS; }

}  // namespace

extern "C" {

int vc_jd_tile(void) { return TILE; }

size_t vc_jd_table_floats(int32_t M, int32_t D) { return shape_ok(M, D) ? table_floats(M, D) : 0; }

size_t vc_jd_workspace_size(int32_t M, int32_t D) {
    if (!shape_ok(M, D)) return 0;
    return vc::align256((size_t)PARTS * ((M + CHUNK - 1) / CHUNK) * blk_doubles(D) * sizeof(double));
}

size_t vc_mlpg_workspace_size(int32_t batch, int32_t max_frames, int32_t n_coef) {
    if (batch < 1 || batch > 65535 || max_frames < 1 || max_frames > MLPG_MAX_F || n_coef < 1 || n_coef > MAX_CEP) return 0;
    return vc::align256((size_t)batch * max_frames * 5 * n_coef * sizeof(VC_MLPG_REAL));
}

int vc_jd_prepare_f32(const float* d_w, const float* d_mu_x, const float* d_mu_y, const float* d_var_x, const float* d_var_y,
                      const float* d_cov_xy, int32_t M, int32_t D, float* d_table, void* stream) {
    VC_REQUIRE(d_w && d_mu_x && d_mu_y && d_var_x && d_var_y && d_cov_xy && d_table, "vc_jd_prepare_f32: NULL argument");
    VC_REQUIRE(M >= 1 && D >= 1, "vc_jd_prepare_f32: bad shape (M %d, D %d)", M, D);
    if (!shape_ok(M, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_jd_prepare_f32: limits are M <= %d, D <= %d; got %d, %d", MAX_M, MAX_D, M, D);
    hipLaunchKernelGGL(jd_prepare_kernel, dim3(blocks_for(table_floats(M, D))), dim3(NT), 0, static_cast<hipStream_t>(stream), d_w,
                       d_mu_x, d_mu_y, d_var_x, d_var_y, d_cov_xy, M, D, d_table);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_jd_accumulate_f32(const float* d_feat_a, const float* d_feat_b, const int32_t* d_len_a, const int32_t* d_len_b,
                         const int32_t* d_path, const int32_t* d_path_len, int32_t batch, int32_t max_a, int32_t max_b,
                         int32_t max_path, int32_t D, const float* d_table, int32_t M, double* d_N, double* d_S, double* d_L,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_feat_a && d_feat_b && d_len_a && d_len_b && d_table && d_N && d_S && d_L, "vc_jd_accumulate_f32: NULL argument");
    VC_REQUIRE((d_path == nullptr) == (d_path_len == nullptr), "vc_jd_accumulate_f32: pass d_path and d_path_len together or neither");
    VC_REQUIRE(batch >= 1 && max_a >= 1 && max_b >= 1 && D >= 1 && M >= 1 && (d_path ? max_path >= 1 : max_path == 0),
               "vc_jd_accumulate_f32: bad arguments (batch %d, max_a %d, max_b %d, max_path %d, D %d, M %d)", batch, max_a, max_b,
               max_path, D, M);
    if (!shape_ok(M, D) || !frames_ok(batch, max_a, D) || !frames_ok(batch, max_b, D) || max_path > MAX_PATH)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_jd_accumulate_f32: limits are M <= %d, D <= %d, batch <= 65535, frames * D <= 2^30 "
                             "and max_path <= 2^24; got %d, %d, batch %d, max_a %d, max_b %d, max_path %d", MAX_M, MAX_D, M, D, batch,
                             max_a, max_b, max_path);
    const size_t need = vc_jd_workspace_size(M, D);
    VC_REQUIRE(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "vc_jd_accumulate_f32: NULL or unaligned workspace");
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_jd_accumulate_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const int chunks = (M + CHUNK - 1) / CHUNK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jd_accumulate_kernel, dim3(chunks, PARTS), dim3(ACC_NT), 0, st, d_feat_a, d_feat_b, d_len_a, d_len_b, d_path,
                       d_path_len, batch, max_a, max_b, max_path, D, d_table, M, static_cast<double*>(d_workspace));
    VC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jd_reduce_kernel, dim3(blocks_for((size_t)M + 5 * (size_t)M * D + 2)), dim3(NT), 0, st,
                       static_cast<const double*>(d_workspace), M, D, chunks, d_N, d_S, d_L);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_jd_update_f32(const double* d_N, const double* d_S, int32_t M, int32_t D, const float* d_mu_x_in, const float* d_mu_y_in,
                     const float* d_var_x_in, const float* d_var_y_in, const float* d_cov_in, const float* d_floor_x,
                     const float* d_floor_y, float rho_max, float min_count, float* d_w_out, float* d_mu_x_out, float* d_mu_y_out,
                     float* d_var_x_out, float* d_var_y_out, float* d_cov_out, void* stream) {
    VC_REQUIRE(d_N && d_S && d_mu_x_in && d_mu_y_in && d_var_x_in && d_var_y_in && d_cov_in && d_floor_x && d_floor_y && d_w_out &&
               d_mu_x_out && d_mu_y_out && d_var_x_out && d_var_y_out && d_cov_out, "vc_jd_update_f32: NULL argument");
    VC_REQUIRE(M >= 1 && D >= 1, "vc_jd_update_f32: bad shape (M %d, D %d)", M, D);
    VC_REQUIRE(rho_max >= 0.0f && rho_max < 1.0f && min_count >= 0.0f, "vc_jd_update_f32: need 0 <= rho_max < 1 and min_count >= 0");
    if (!shape_ok(M, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_jd_update_f32: limits are M <= %d, D <= %d; got %d, %d", MAX_M, MAX_D, M, D);
    hipLaunchKernelGGL(jd_update_kernel, dim3(blocks_for((size_t)M * D)), dim3(NT), 0, static_cast<hipStream_t>(stream), d_N, d_S, M, D,
                       d_mu_x_in, d_mu_y_in, d_var_x_in, d_var_y_in, d_cov_in, d_floor_x, d_floor_y, rho_max, min_count, d_w_out,
                       d_mu_x_out, d_mu_y_out, d_var_x_out, d_var_y_out, d_cov_out);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_jd_map_f32(const float* d_feat, const int32_t* d_len, int32_t batch, int32_t max_frames, int32_t D, const float* d_table,
                  int32_t M, int32_t mixture, float* d_P, float* d_R, float* d_mmse, int32_t* d_best, void* stream) {
    VC_REQUIRE(d_feat && d_len && d_table && d_P && d_R, "vc_jd_map_f32: NULL argument");
    VC_REQUIRE(mixture == 0 || (mixture == 1 && d_best), "vc_jd_map_f32: mixture must be 0 (soft) or 1 (best, with d_best)");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && D >= 1 && M >= 1, "vc_jd_map_f32: bad shape (batch %d, max_frames %d, D %d, M %d)", batch,
               max_frames, D, M);
    if (!shape_ok(M, D) || !frames_ok(batch, max_frames, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_jd_map_f32: limits are M <= %d, D <= %d, batch <= 65535 and max_frames * D <= 2^30; "
                             "got %d, %d, batch %d, max_frames %d", MAX_M, MAX_D, M, D, batch, max_frames);
    hipLaunchKernelGGL(jd_map_kernel, dim3((max_frames + TILE - 1) / TILE, batch), dim3(MAP_NT), 0, static_cast<hipStream_t>(stream),
                       d_feat, d_len, max_frames, D, d_table, M, mixture, d_P, d_R, d_mmse, d_best);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_mlpg_f32(const float* d_P, const float* d_R, const int32_t* d_len, int32_t batch, int32_t max_frames, int32_t n_coef,
                float* d_y, int32_t* d_flags, void* d_workspace, size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_P && d_R && d_len && d_y && d_flags, "vc_mlpg_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_coef >= 1, "vc_mlpg_f32: bad shape (batch %d, max_frames %d, n_coef %d)", batch,
               max_frames, n_coef);
    const size_t need = vc_mlpg_workspace_size(batch, max_frames, n_coef);
    if (need == 0)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_mlpg_f32: limits are batch <= 65535, max_frames <= 2^20, n_coef <= %d; got %d, %d, %d",
                             MAX_CEP, batch, max_frames, n_coef);
    VC_REQUIRE(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "vc_mlpg_f32: NULL or unaligned workspace");
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_mlpg_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipLaunchKernelGGL(mlpg_kernel<VC_MLPG_REAL>, dim3(batch), dim3(64), 0, static_cast<hipStream_t>(stream), d_P, d_R, d_len, max_frames,
                       n_coef, d_y, d_flags, static_cast<VC_MLPG_REAL*>(d_workspace));
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_cep_gain_f32(const float* d_cep_pred, const float* d_cep_src, const int32_t* d_n_frames, int32_t batch, int32_t max_frames,
                    int32_t n_coef, const float* d_dct, int32_t n_mels, const int32_t* d_bin_i0, const float* d_bin_w, int32_t n_bins,
                    float alpha, float db_scale, float max_boost_db, float max_cut_db, float* d_gain, void* stream) {
    VC_REQUIRE(d_cep_pred && d_cep_src && d_dct && d_bin_i0 && d_bin_w && d_gain, "vc_cep_gain_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_coef >= 1 && n_mels >= 2 && n_bins >= 1,
               "vc_cep_gain_f32: bad shape (batch %d, max_frames %d, n_coef %d, n_mels %d, n_bins %d)", batch, max_frames, n_coef, n_mels,
               n_bins);
    VC_REQUIRE(alpha >= 0.0f && alpha <= 1.0f && std::isfinite(db_scale) && max_boost_db >= 0.0f && std::isfinite(max_boost_db) &&
               max_cut_db >= 0.0f && std::isfinite(max_cut_db),
               "vc_cep_gain_f32: need alpha in [0, 1], a finite db_scale and finite max_boost_db, max_cut_db >= 0");
    if (batch > 65535 || n_coef > MAX_CEP || n_coef > n_mels || n_mels > GAIN_MAX_MELS || n_bins > GAIN_MAX_BINS ||
        (int64_t)max_frames * n_bins > MAX_ELEMS)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_cep_gain_f32: limits are batch <= 65535, n_coef <= min(%d, n_mels), n_mels <= %d, "
                             "n_bins <= %d, max_frames * n_bins <= 2^30; got %d, %d, %d, %d, max_frames %d", MAX_CEP, GAIN_MAX_MELS,
                             GAIN_MAX_BINS, batch, n_coef, n_mels, n_bins, max_frames);
    hipLaunchKernelGGL(cep_gain_kernel, dim3((max_frames + GAIN_TILE - 1) / GAIN_TILE, batch), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), d_cep_pred, d_cep_src, d_n_frames, max_frames, n_coef, d_dct, n_mels, d_bin_i0,
                       d_bin_w, n_bins, alpha, db_scale, max_boost_db, max_cut_db, d_gain);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
