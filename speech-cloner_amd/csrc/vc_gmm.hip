// Speaker similarity on the device (include/vc_hip.h, "Speaker"): a diagonal-covariance Gaussian mixture over cepstral
// features -- the universal background model (UBM) --, models of single speakers whose means are MAP-adapted from it, and
// the mean per-frame log-likelihood ratio of an utterance between a speaker's model and the UBM.
//
//     l_m(x)  = c_m - 0.5 * sum_d (x_d - mu_md)^2 / var_md,   c_m = log w_m - 0.5 * sum_d log(2 pi var_md)
//     ll(x)   = max_m l_m + log sum_m exp(l_m - max)
//     gamma_m = exp(l_m - ll)                                  the responsibility of component m for frame x
//
// spk_features_kernel: one workgroup of 256 lanes per utterance.  Lane t owns column t & 63 and the frames (t >> 6),
// (t >> 6) + 4, ...; the column sums of the kept frames are float64, a lane's frames ascending, then the four lanes of a
// column in the order 0 .. 3.  A second walk writes feature - mean (the feature is formed again, not read back).
//
// gmm_prepare_kernel: the table the other kernels read -- means and 1 / var TRANSPOSED to [d][m], so that lane m of a wave
// reads consecutive words for every d, and c_m.  No kernel keeps parameters in LDS: they stay in L2 / L1.
//
// gmm_loglik_kernel: one workgroup of 256 lanes per (utterance, tile of 32 frames).  The tile's features go to LDS; lane m
// is component m and forms l_m for eight frames at a time (one read of mu and 1 / var per d serves eight chains of fused
// multiply-adds); the l_m of the tile go to LDS [frame][component]; then one wave per frame: lane l takes components l,
// l + 64, ... ascending, maximum and sum by butterflies.  A second model per utterance reuses the tile.
//
// gmm_accumulate_kernel: the E-step without the posterior matrix.  Grid = (chunks of 64 components) x (P partitions) x
// (G groups), P = vc_gmm_partitions(G) = max(1, 128 / G): a function of the arguments, never of the device.  Workgroup
// (c, p, g) walks the utterances b = 0, 1, ... of group g and of each the tiles k with (b + k) % P == p, ascending.  Per
// tile: features, ll and the keep flags to LDS; lane (m = t & 63, r = t >> 6) forms gamma of component 64 c + m for frames
// 8 r .. 8 r + 7 into LDS [frame][m]; then lane (m, q = t >> 6) adds, frame by frame (a frame the mask drops is skipped:
// its features may hold anything), gamma * x and gamma * x^2 of the dimensions d = q, q + 4, ... into float64 REGISTERS (at most 16 dimensions, 32 accumulators and N: the accumulators
// never touch LDS, whose banks then carry only the float32 tile: gamma read lane-consecutive, x as a broadcast).  One
// partial block per workgroup at the end; gmm_reduce_kernel adds the partitions of an element in the order 0 .. P - 1.
// With P = 1 (G > 64) the workgroup writes the outputs itself and there is no workspace.
//
// gmm_score_kernel: one workgroup of 256 lanes per utterance, lane t adds frames t, t + 256, ... in float64, then a fixed
// tree over the 256 partial sums.
//
// gmm_update_kernel: elementwise over (model, component, dimension), float64, each output rounded once.
//
// No atomics, no memset, no hand-off between workgroups; fixed geometry and fixed orders: every output is bit-identical
// from run to run and under graph replay, and the score figures of an utterance do not depend on its batch.
#include <cmath>
#include "vc_device.h"

namespace {

constexpr int MAX_M = 256;
constexpr int MAX_D = 64;
constexpr int MAX_S = 4096;            // groups; a table holds MAX_S speaker models and the UBM
constexpr int MAX_CEP = 32;
constexpr int MAX_ELEMS = 1 << 30;      // frames * D of one utterance
constexpr int TILE = 32;                // frames per tile, loglik and accumulate
constexpr int NT = 256;
constexpr int CHUNK = 64;               // components per accumulate workgroup
constexpr int PARTS = 128;              // frame partitions of one group when G = 1
constexpr int DQ = MAX_D / 4;           // dimensions per lane of the accumulate kernel

inline int n_parts(int G) { return G >= PARTS ? 1 : PARTS / G; }
__host__ __device__ inline size_t blk_doubles(int D) { return (size_t)CHUNK * (1 + 2 * D) + 1; }

// ------------------------------------------------------------------------------------------------------------ features
__device__ inline float feat_value(const float* __restrict__ C, int n_coef, int len, int f, int col) {
    if (col < n_coef) return C[(size_t)f * n_coef + col];
    const int k = col - n_coef;
    const int p1 = min(f + 1, len - 1), m1 = max(f - 1, 0), p2 = min(f + 2, len - 1), m2 = max(f - 2, 0);
    const float d1 = C[(size_t)p1 * n_coef + k] - C[(size_t)m1 * n_coef + k];
    const float d2 = C[(size_t)p2 * n_coef + k] - C[(size_t)m2 * n_coef + k];
    return fmaf(2.0f, d2, d1) / 10.0f;
}

__global__ void __launch_bounds__(NT)
spk_features_kernel(const float* __restrict__ cep, const int32_t* __restrict__ lens, const uint8_t* __restrict__ mask, int max_frames,
                    int n_coef, int D, int cmn, float* __restrict__ out) {
    __shared__ double part[4][64];
    __shared__ int cnt[4];
    const int b = blockIdx.x, t = threadIdx.x, col = t & 63, r = t >> 6;
    const int len = min(max(lens[b], 0), max_frames);
    const float* __restrict__ C = cep + (size_t)b * max_frames * n_coef;
    const uint8_t* __restrict__ K = mask ? mask + (size_t)b * max_frames : nullptr;
    float* __restrict__ O = out + (size_t)b * max_frames * D;
    float mean = 0.0f;
    if (cmn) {
        double s = 0.0;
        int n = 0;
        for (int f = r; f < len; f += 4) {
            if (K && !K[f]) continue;
            ++n;
            if (col < D) s += (double)feat_value(C, n_coef, len, f, col);
        }
        part[r][col] = s;
        if (col == 0) cnt[r] = n;
        __syncthreads();
        const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        const double sum = ((part[0][col] + part[1][col]) + part[2][col]) + part[3][col];
        if (total > 0) mean = (float)(sum / (double)total);
    }
    if (col < D) {
        for (int f = r; f < max_frames; f += 4)
            O[(size_t)f * D + col] = f < len ? feat_value(C, n_coef, len, f, col) - mean : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------- prepare
// table: muT [S][D][M], ivarT [D][M], c [M]
__global__ void __launch_bounds__(NT)
gmm_prepare_kernel(const float* __restrict__ w, const float* __restrict__ mu, const float* __restrict__ var, int S, int M, int D,
                   float* __restrict__ table) {
    const size_t n_mu = (size_t)S * M * D, n_iv = (size_t)M * D;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < n_mu) {                                                 // i indexes the output [s][d][m]
        const int m = (int)(i % M), d = (int)((i / M) % D);
        const size_t s = i / ((size_t)M * D);
        table[i] = mu[(s * M + m) * D + d];
    } else if (i < n_mu + n_iv) {
        const size_t j = i - n_mu;
        const int m = (int)(j % M), d = (int)(j / M);
        table[i] = (float)(1.0 / (double)var[(size_t)m * D + d]);
    } else if (i < n_mu + n_iv + M) {
        const int m = (int)(i - n_mu - n_iv);
        double acc = 0.0;
        for (int d = 0; d < D; ++d) acc += log(6.283185307179586476925 * (double)var[(size_t)m * D + d]);
        table[i] = (float)(log((double)w[m]) - 0.5 * acc);
    }
}

// q[j] = sum_d (x[f0 + j][d] - mu_d)^2 * ivar_d for eight frames of the LDS tile xs [TILE][D], d ascending
__device__ inline void quad8(const float* __restrict__ xs, int D, int f0, const float* __restrict__ muT, const float* __restrict__ ivT,
                             int M, int m, float (&q)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float mu = muT[(size_t)d * M + m], iv = ivT[(size_t)d * M + m];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float df = xs[(f0 + j) * D + d] - mu;
            q[j] = fmaf(df * df, iv, q[j]);
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- loglik
__global__ void __launch_bounds__(NT)
gmm_loglik_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int max_frames, int D, const float* __restrict__ table,
                  int S, int M, const int32_t* __restrict__ model_a, const int32_t* __restrict__ model_b, float* __restrict__ ll_a,
                  float* __restrict__ ll_b) {
    __shared__ float xs[TILE * MAX_D];
    __shared__ float lbuf[TILE * MAX_M];
    const int b = blockIdx.y, f0 = blockIdx.x * TILE, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int len = min(max(lens[b], 0), max_frames);
    const int nf = min(TILE, len - f0);                             // frames of this tile below len
    const int n_out = min(TILE, max_frames - f0);
    float* __restrict__ out_a = ll_a + (size_t)b * max_frames + f0;
    float* __restrict__ out_b = ll_b ? ll_b + (size_t)b * max_frames + f0 : nullptr;
    if (nf <= 0) {
        if (t < n_out) {
            out_a[t] = 0.0f;
            if (out_b) out_b[t] = 0.0f;
        }
        return;
    }
    const float* __restrict__ X = x + ((size_t)b * max_frames + f0) * D;
    for (int i = t; i < TILE * D; i += NT) xs[i] = i < nf * D ? X[i] : 0.0f;
    const float* __restrict__ ivT = table + (size_t)S * D * M;
    const float* __restrict__ cc = ivT + (size_t)D * M;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !out_b) break;
        float* __restrict__ out = pass ? out_b : out_a;
        const int s = min(max((pass ? model_b : model_a)[b], 0), S - 1);
        const float* __restrict__ muT = table + (size_t)s * D * M;
        __syncthreads();                                            // xs filled; the previous pass's reads of lbuf
        if (t < M) {
            const float c = cc[t];
            for (int g0 = 0; g0 < nf; g0 += 8) {
                float q[8];
                quad8(xs, D, g0, muT, ivT, M, t, q);
#pragma unroll
                for (int j = 0; j < 8; ++j) lbuf[(g0 + j) * MAX_M + t] = fmaf(-0.5f, q[j], c);
            }
        }
        __syncthreads();
        for (int f = wave; f < n_out; f += NT / 64) {               // uniform over the wave
            float res = 0.0f;
            if (f < nf) {
                float v[MAX_M / 64];
                float mx = -__builtin_inff();
#pragma unroll
                for (int k = 0; k < MAX_M / 64; ++k) {
                    v[k] = lane + 64 * k < M ? lbuf[f * MAX_M + lane + 64 * k] : -__builtin_inff();
                    mx = fmaxf(mx, v[k]);
                }
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sh, 64));
                float sum = 0.0f;
#pragma unroll
                for (int k = 0; k < MAX_M / 64; ++k)
                    if (lane + 64 * k < M) sum += expf(v[k] - mx);
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh, 64);
                res = mx + logf(sum);
            }
            if (lane == 0) out[f] = res;
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- score
__global__ void __launch_bounds__(NT)
gmm_score_kernel(const float* __restrict__ ll_a, const float* __restrict__ ll_b, const int32_t* __restrict__ lens,
                 const uint8_t* __restrict__ mask, int max_frames, int32_t* __restrict__ n_frames, float* __restrict__ values) {
    __shared__ double sa[NT], sb[NT];
    __shared__ int sn[NT];
    const int b = blockIdx.x, t = threadIdx.x;
    const int len = min(max(lens[b], 0), max_frames);
    const float* __restrict__ A = ll_a + (size_t)b * max_frames;
    const float* __restrict__ Bp = ll_b ? ll_b + (size_t)b * max_frames : nullptr;
    const uint8_t* __restrict__ K = mask ? mask + (size_t)b * max_frames : nullptr;
    double a = 0.0, c = 0.0;
    int n = 0;
    for (int f = t; f < len; f += NT) {
        if (K && !K[f]) continue;
        ++n;
        a += (double)A[f];
        if (Bp) c += (double)Bp[f];
    }
    sa[t] = a;
    sb[t] = c;
    sn[t] = n;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) { sa[t] += sa[t + s]; sb[t] += sb[t + s]; sn[t] += sn[t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        const float nan = __builtin_nanf("");
        const int cnt = sn[0];
        n_frames[b] = cnt;
        values[3 * b] = cnt > 0 ? (float)(sa[0] / (double)cnt) : nan;
        values[3 * b + 1] = cnt > 0 && Bp ? (float)(sb[0] / (double)cnt) : nan;
        values[3 * b + 2] = cnt > 0 && Bp ? (float)(sa[0] / (double)cnt - sb[0] / (double)cnt) : nan;
    }
}

// ---------------------------------------------------------------------------------------------------------- accumulate
// dst: the partial block of this workgroup (direct = 0: [CHUNK] N, [CHUNK][D] S1, [CHUNK][D] S2, L) or the outputs.
__global__ void __launch_bounds__(NT)
gmm_accumulate_kernel(const float* __restrict__ x, const float* __restrict__ ll, const int32_t* __restrict__ lens,
                      const uint8_t* __restrict__ mask, const int32_t* __restrict__ group, int batch, int max_frames, int D,
                      const float* __restrict__ table, int S, int M, int model, int P, int direct, double* __restrict__ ws,
                      double* __restrict__ outN, double* __restrict__ outS1, double* __restrict__ outS2, double* __restrict__ outL) {
    __shared__ float xs[TILE * MAX_D];
    __shared__ float gam[TILE * CHUNK];
    __shared__ float lls[TILE];
    __shared__ int keep[TILE];
    const int c = blockIdx.x, p = blockIdx.y, g = blockIdx.z, t = threadIdx.x;
    const int ml = t & 63, r = t >> 6;
    const int m = c * CHUNK + ml;
    const float* __restrict__ muT = table + (size_t)model * D * M;
    const float* __restrict__ ivT = table + (size_t)S * D * M;
    const float cm = m < M ? ivT[(size_t)D * M + m] : 0.0f;
    double s1[DQ], s2[DQ];
#pragma unroll
    for (int j = 0; j < DQ; ++j) s1[j] = s2[j] = 0.0;
    double nsum = 0.0, lsum = 0.0;
    for (int b = 0; b < batch; ++b) {                               // uniform over the workgroup
        if (group[b] != g) continue;
        const int len = min(max(lens[b], 0), max_frames);
        const int n_tiles = (len + TILE - 1) / TILE;
        int k = (p - b % P + P) % P;                                // the first tile with (b + k) % P == p
        for (; k < n_tiles; k += P) {
            const int f0 = k * TILE;
            const int nf = min(TILE, len - f0);
            const float* __restrict__ X = x + ((size_t)b * max_frames + f0) * D;
            __syncthreads();                                        // the previous tile's reads
            for (int i = t; i < TILE * D; i += NT) xs[i] = i < nf * D ? X[i] : 0.0f;
            if (t < TILE) {
                const bool kp = t < nf && (!mask || mask[(size_t)b * max_frames + f0 + t]);
                keep[t] = kp ? 1 : 0;
                lls[t] = t < nf ? ll[(size_t)b * max_frames + f0 + t] : 0.0f;
            }
            __syncthreads();
            {
                float q[8] = {};
                if (m < M) quad8(xs, D, 8 * r, muT, ivT, M, m, q);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int f = 8 * r + j;
                    gam[f * CHUNK + ml] = m < M && keep[f] ? expf(fmaf(-0.5f, q[j], cm) - lls[f]) : 0.0f;
                }
            }
            __syncthreads();
            for (int f = 0; f < nf; ++f) {
                if (!keep[f]) continue;                             // uniform over the workgroup; a dropped frame's x is not used
                const double gm = (double)gam[f * CHUNK + ml];
                if (r == 0) nsum += gm;
#pragma unroll
                for (int j = 0; j < DQ; ++j) {
                    const int d = r + 4 * j;
                    if (d < D) {
                        const double xv = (double)xs[f * D + d];
                        const double gx = gm * xv;
                        s1[j] += gx;
                        s2[j] = fma(gx, xv, s2[j]);
                    }
                }
            }
            if (t == 0 && c == 0)
                for (int f = 0; f < nf; ++f)
                    if (keep[f]) lsum += (double)lls[f];
        }
    }
    // where this lane's sums go: the outputs themselves (one partition) or the workgroup's partial block
    double *pN, *pS1, *pS2, *pL;
    bool mine, first;
    if (direct) {
        pN = outN + (size_t)g * M + m;
        pS1 = outS1 + ((size_t)g * M + m) * D;
        pS2 = outS2 + ((size_t)g * M + m) * D;
        pL = outL + g;
        mine = m < M;
        first = t == 0 && c == 0;
    } else {
        double* blk = ws + (((size_t)g * P + p) * gridDim.x + c) * blk_doubles(D);
        pN = blk + ml;
        pS1 = blk + CHUNK + (size_t)ml * D;
        pS2 = pS1 + (size_t)CHUNK * D;
        pL = blk + CHUNK + 2 * (size_t)CHUNK * D;
        mine = true;
        first = t == 0;
    }
    if (mine) {
        if (r == 0) *pN = nsum;
#pragma unroll
        for (int j = 0; j < DQ; ++j) {
            const int d = r + 4 * j;
            if (d < D) {
                pS1[d] = s1[j];
                pS2[d] = s2[j];
            }
        }
    }
    if (first) *pL = lsum;
}

// out element e of group g: e < M: N; e < M + M D: S1; e < M + 2 M D: S2; e == M + 2 M D: L
__global__ void __launch_bounds__(NT)
gmm_reduce_kernel(const double* __restrict__ ws, int G, int M, int D, int P, int chunks, double* __restrict__ outN,
                  double* __restrict__ outS1, double* __restrict__ outS2, double* __restrict__ outL) {
    const size_t per = (size_t)M + 2 * (size_t)M * D + 1;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= per * G) return;
    const int g = (int)(i / per);
    const size_t e = i % per;
    const size_t MD = (size_t)M * D;
    int m;
    size_t off;                                                     // inside a partial block
    double* dst;
    if (e < (size_t)M) {
        m = (int)e;
        off = m % CHUNK;
        dst = outN + (size_t)g * M + m;
    } else if (e < M + MD) {
        const size_t j = e - M;
        m = (int)(j / D);
        off = CHUNK + (size_t)(m % CHUNK) * D + j % D;
        dst = outS1 + (size_t)g * MD + j;
    } else if (e < M + 2 * MD) {
        const size_t j = e - M - MD;
        m = (int)(j / D);
        off = CHUNK + (size_t)CHUNK * D + (size_t)(m % CHUNK) * D + j % D;
        dst = outS2 + (size_t)g * MD + j;
    } else {
        m = 0;
        off = CHUNK + 2 * (size_t)CHUNK * D;
        dst = outL + g;
    }
    const int c = m / CHUNK;
    double acc = 0.0;
    for (int p = 0; p < P; ++p) acc += ws[(((size_t)g * P + p) * chunks + c) * blk_doubles(D) + off];
    *dst = acc;
}

// -------------------------------------------------------------------------------------------------------------- update
__global__ void __launch_bounds__(NT)
gmm_update_kernel(int mode, const double* __restrict__ N, const double* __restrict__ S1, const double* __restrict__ S2, int G, int M,
                  int D, const float* __restrict__ mu_in, const float* __restrict__ var_in, const float* __restrict__ var_floor,
                  float min_count, float relevance, float* __restrict__ w_out, float* __restrict__ mu_out, float* __restrict__ var_out) {
    const size_t MD = (size_t)M * D;
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= MD * G) return;
    const size_t j = i % MD;                                        // (m, d) inside the model
    const int g = (int)(i / MD), m = (int)(j / D), d = (int)(j % D);
    const double n = N[(size_t)g * M + m];
    if (mode == 0) {                                                // EM, G = 1
        if (d == 0) {
            double tot = 0.0;
            for (int k = 0; k < M; ++k) tot += N[k];
            const double wv = n / tot;
            w_out[m] = (float)(wv > 0x1p-40 ? wv : 0x1p-40);        // (a NaN quotient, no frame at all, gives the floor)
        }
        if (n < (double)min_count) {
            mu_out[j] = mu_in[j];
            var_out[j] = var_in[j];
        } else {
            const double mean = S1[j] / n;
            const double v = S2[j] / n - mean * mean;
            const double fl = (double)var_floor[d];
            mu_out[j] = (float)mean;
            var_out[j] = (float)(v > fl ? v : fl);
        }
    } else {                                                        // MAP, means only
        if (n > 0.0) {
            const double alpha = n / (n + (double)relevance);
            mu_out[i] = (float)(alpha * (S1[i] / n) + (1.0 - alpha) * (double)mu_in[j]);
        } else {
            mu_out[i] = mu_in[j];
        }
    }
}

inline bool gmm_shape_ok(int S, int M, int D) { return S <= MAX_S + 1 && M <= MAX_M && D <= MAX_D; }
inline bool frames_ok(int batch, int max_frames, int D) { return batch <= 65535 && (int64_t)max_frames * D <= MAX_ELEMS; }
inline unsigned blocks_for(size_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

extern "C" {

int vc_gmm_tile_frames(void) { return TILE; }

int vc_gmm_partitions(int32_t n_groups) { return n_groups >= 1 && n_groups <= MAX_S ? n_parts(n_groups) : 0; }

size_t vc_gmm_table_floats(int32_t n_models, int32_t M, int32_t D) {
    if (n_models < 1 || M < 1 || D < 1 || !gmm_shape_ok(n_models, M, D)) return 0;
    return ((size_t)n_models + 1) * M * D + M;
}

size_t vc_gmm_workspace_bytes(int32_t n_groups, int32_t M, int32_t D) {
    if (n_groups < 1 || n_groups > MAX_S || M < 1 || D < 1 || !gmm_shape_ok(n_groups, M, D)) return 0;
    const int P = n_parts(n_groups);
    if (P == 1) return 0;
    return vc::align256((size_t)n_groups * P * ((M + CHUNK - 1) / CHUNK) * blk_doubles(D) * sizeof(double));
}

int vc_spk_features_f32(const float* d_cep, const int32_t* d_len, const uint8_t* d_mask, int32_t batch, int32_t max_frames,
                        int32_t n_coef, int32_t deltas, int32_t cmn, float* d_feat, void* stream) {
    VC_REQUIRE(d_cep && d_len && d_feat, "vc_spk_features_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_coef >= 1 && (deltas == 0 || deltas == 1) && (cmn == 0 || cmn == 1),
               "vc_spk_features_f32: bad arguments (batch %d, max_frames %d, n_coef %d, deltas %d, cmn %d)", batch, max_frames, n_coef,
               deltas, cmn);
    const int D = n_coef * (1 + deltas);
    if (n_coef > MAX_CEP || !frames_ok(batch, max_frames, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_spk_features_f32: limits are n_coef <= %d, batch <= 65535 and max_frames * D <= "
                             "2^30; got n_coef %d, batch %d, max_frames %d, D %d", MAX_CEP, n_coef, batch, max_frames, D);
    hipLaunchKernelGGL(spk_features_kernel, dim3(batch), dim3(NT), 0, static_cast<hipStream_t>(stream), d_cep, d_len, d_mask, max_frames,
                       n_coef, D, cmn, d_feat);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_gmm_prepare_f32(const float* d_w, const float* d_mu, const float* d_var, int32_t n_models, int32_t M, int32_t D, float* d_table,
                       void* stream) {
    VC_REQUIRE(d_w && d_mu && d_var && d_table, "vc_gmm_prepare_f32: NULL argument");
    VC_REQUIRE(n_models >= 1 && M >= 1 && D >= 1, "vc_gmm_prepare_f32: bad shape (n_models %d, M %d, D %d)", n_models, M, D);
    if (!gmm_shape_ok(n_models, M, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_gmm_prepare_f32: limits are n_models <= %d, M <= %d, D <= %d; got %d, %d, %d", MAX_S + 1,
                             MAX_M, MAX_D, n_models, M, D);
    hipLaunchKernelGGL(gmm_prepare_kernel, dim3(blocks_for(vc_gmm_table_floats(n_models, M, D))), dim3(NT), 0,
                       static_cast<hipStream_t>(stream), d_w, d_mu, d_var, n_models, M, D, d_table);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_gmm_loglik_f32(const float* d_feat, const int32_t* d_len, int32_t batch, int32_t max_frames, int32_t D, const float* d_table,
                      int32_t n_models, int32_t M, const int32_t* d_model, float* d_ll, const int32_t* d_model_b, float* d_ll_b,
                      void* stream) {
    VC_REQUIRE(d_feat && d_len && d_table && d_model && d_ll, "vc_gmm_loglik_f32: NULL argument");
    VC_REQUIRE((d_model_b == nullptr) == (d_ll_b == nullptr), "vc_gmm_loglik_f32: pass d_model_b and d_ll_b together or neither");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && D >= 1 && n_models >= 1 && M >= 1,
               "vc_gmm_loglik_f32: bad shape (batch %d, max_frames %d, D %d, n_models %d, M %d)", batch, max_frames, D, n_models, M);
    if (!gmm_shape_ok(n_models, M, D) || !frames_ok(batch, max_frames, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_gmm_loglik_f32: limits are n_models <= %d, M <= %d, D <= %d, batch <= 65535 and "
                             "max_frames * D <= 2^30; got %d, %d, %d, batch %d, max_frames %d", MAX_S + 1, MAX_M, MAX_D, n_models, M, D, batch,
                             max_frames);
    hipLaunchKernelGGL(gmm_loglik_kernel, dim3((max_frames + TILE - 1) / TILE, batch), dim3(NT), 0, static_cast<hipStream_t>(stream),
                       d_feat, d_len, max_frames, D, d_table, n_models, M, d_model, d_model_b, d_ll, d_ll_b);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_gmm_score_f32(const float* d_ll_a, const float* d_ll_b, const int32_t* d_len, const uint8_t* d_mask, int32_t batch,
                     int32_t max_frames, int32_t* d_n_frames, float* d_values, void* stream) {
    VC_REQUIRE(d_ll_a && d_len && d_n_frames && d_values, "vc_gmm_score_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1, "vc_gmm_score_f32: bad shape (batch %d, max_frames %d)", batch, max_frames);
    if (!frames_ok(batch, max_frames, 1))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_gmm_score_f32: limits are batch <= 65535 and max_frames <= 2^30; got %d, %d", batch,
                             max_frames);
    hipLaunchKernelGGL(gmm_score_kernel, dim3(batch), dim3(NT), 0, static_cast<hipStream_t>(stream), d_ll_a, d_ll_b, d_len, d_mask,
                       max_frames, d_n_frames, d_values);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_gmm_accumulate_f32(const float* d_feat, const float* d_ll, const int32_t* d_len, const uint8_t* d_mask, const int32_t* d_group,
                          int32_t batch, int32_t max_frames, int32_t D, const float* d_table, int32_t n_models, int32_t M, int32_t model,
                          int32_t n_groups, double* d_N, double* d_S1, double* d_S2, double* d_L, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_feat && d_ll && d_len && d_group && d_table && d_N && d_S1 && d_S2 && d_L, "vc_gmm_accumulate_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && D >= 1 && n_models >= 1 && M >= 1 && n_groups >= 1 && model >= 0 && model < n_models,
               "vc_gmm_accumulate_f32: bad arguments (batch %d, max_frames %d, D %d, n_models %d, M %d, model %d, n_groups %d)", batch,
               max_frames, D, n_models, M, model, n_groups);
    if (!gmm_shape_ok(n_models, M, D) || n_groups > MAX_S || !frames_ok(batch, max_frames, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_gmm_accumulate_f32: limits are n_models - 1, n_groups <= %d, M <= %d, D <= %d, batch <= "
                             "65535 and max_frames * D <= 2^30; got %d, %d, %d, %d, batch %d, max_frames %d", MAX_S, MAX_M, MAX_D, n_models,
                             n_groups, M, D, batch, max_frames);
    const size_t need = vc_gmm_workspace_bytes(n_groups, M, D);
    if (need) {
        VC_REQUIRE(d_workspace && (reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "vc_gmm_accumulate_f32: NULL or unaligned workspace");
        if (workspace_bytes < need)
            return vc::set_error(VC_ERR_WORKSPACE, "vc_gmm_accumulate_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    }
    const int P = n_parts(n_groups), chunks = (M + CHUNK - 1) / CHUNK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gmm_accumulate_kernel, dim3(chunks, P, n_groups), dim3(NT), 0, st, d_feat, d_ll, d_len, d_mask, d_group, batch,
                       max_frames, D, d_table, n_models, M, model, P, P == 1 ? 1 : 0, static_cast<double*>(d_workspace), d_N, d_S1, d_S2,
                       d_L);
    VC_HIP_CHECK(hipGetLastError());
    if (P > 1) {
        const size_t per = (size_t)M + 2 * (size_t)M * D + 1;
        hipLaunchKernelGGL(gmm_reduce_kernel, dim3(blocks_for(per * n_groups)), dim3(NT), 0, st, static_cast<const double*>(d_workspace),
                           n_groups, M, D, P, chunks, d_N, d_S1, d_S2, d_L);
        VC_HIP_CHECK(hipGetLastError());
    }
    return VC_OK;
}

int vc_gmm_update_f32(int32_t mode, const double* d_N, const double* d_S1, const double* d_S2, int32_t n_groups, int32_t M, int32_t D,
                      const float* d_mu_in, const float* d_var_in, const float* d_var_floor, float min_count, float relevance,
                      float* d_w_out, float* d_mu_out, float* d_var_out, void* stream) {
    VC_REQUIRE(mode == 0 || mode == 1, "vc_gmm_update_f32: mode must be 0 (EM) or 1 (MAP), got %d", mode);
    VC_REQUIRE(d_N && d_S1 && d_mu_in && d_mu_out, "vc_gmm_update_f32: NULL argument");
    VC_REQUIRE(n_groups >= 1 && M >= 1 && D >= 1, "vc_gmm_update_f32: bad shape (n_groups %d, M %d, D %d)", n_groups, M, D);
    if (mode == 0) {
        VC_REQUIRE(n_groups == 1, "vc_gmm_update_f32: the EM mode takes one group, got %d", n_groups);
        VC_REQUIRE(d_S2 && d_var_in && d_var_floor && d_w_out && d_var_out, "vc_gmm_update_f32: NULL argument (EM mode)");
        VC_REQUIRE(min_count >= 0.0f, "vc_gmm_update_f32: min_count must be >= 0");
    } else {
        VC_REQUIRE(relevance >= 0.0f && std::isfinite(relevance), "vc_gmm_update_f32: relevance must be finite and >= 0");
    }
    if (n_groups > MAX_S || !gmm_shape_ok(n_groups, M, D))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_gmm_update_f32: limits are n_groups <= %d, M <= %d, D <= %d; got %d, %d, %d", MAX_S,
                             MAX_M, MAX_D, n_groups, M, D);
    hipLaunchKernelGGL(gmm_update_kernel, dim3(blocks_for((size_t)n_groups * M * D)), dim3(NT), 0, static_cast<hipStream_t>(stream), mode,
                       d_N, d_S1, d_S2, n_groups, M, D, d_mu_in, d_var_in, d_var_floor, min_count, relevance, d_w_out, d_mu_out, d_var_out);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
