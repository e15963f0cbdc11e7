// Intelligibility of a time-aligned pair (include/vc_hip.h, "Intelligibility"): STOI (Taal et al. 2011), ESTOI (Jensen &
// Taal 2016) and SI-SDR (Le Roux et al. 2019).  fs = 10 kHz, frames of W = 256 at hop H = 128, a 512-point transform,
// segments of N = 30 frames; the band table is an argument.
//
//   stoi_energy_kernel   e[f] = sum ((x[fH + n] w[n])^2) of the reference and the frame counts.  One wave per frame, four
//                        waves and 16 frames per workgroup; lane l takes samples l, l + 64, l + 128, l + 192 in that order,
//                        then a butterfly over the 64 lanes (the same tree in every lane).
//   stoi_keep_kernel     kept frames e > float32(ratio * max e), ascending, and their count K.  One workgroup of 1,024
//                        lanes per utterance, lane t owns frames [tC, (t + 1)C), C = ceil(F / 1024) <= 16; the position in the
//                        list is a Hillis-Steele sum scan in LDS.  No frame above the threshold (digital silence): K = 0.
//   stoi_bands_kernel    T[sig, b, m, j].  Frame m of the silence-removed signal is never built in memory: its first half is
//                        the second half of kept frame m - 1 plus the first half of kept frame m, its second half the second
//                        half of m plus the first half of m + 1, each windowed, and the sum is windowed again.  One wave
//                        per (signal, utterance, frame), four frames per workgroup.  The 512-point transform is a radix-2
//                        Stockham autosort in LDS, two float2 buffers of 512 per wave: butterfly j of every stage reads
//                        elements j and j + 256, so the 64 lanes of a wave read 64 consecutive float2 (no bank conflict),
//                        and writes q + 2sp and q + 2sp + s (s the stage's stride, p = j / s, q = j % s): two-way conflicts
//                        on the writes of the stages with s < 64, none from there on.  The upper half of the input is zero,
//                        so the first stage is a copy and one product straight from the registers that hold the frame.
//                        Window and twiddles are computed in float64 by the workgroup (one value of each per lane) and
//                        rounded once.  The band sums run over |X[k]|^2 ascending in k, one lane per band.
//   stoi_seg_kernel      seg[b, s] from T: 32 lanes per segment, eight segments per workgroup; the tile's 8 + 29 rows of T
//                        are staged in LDS once.  STOI: lane j takes band j.  ESTOI: lane j takes band j (mean and norm along
//                        time), then lane n takes frame n (mean, norm and product along bands).  Sums ascending from +0.
//   stoi_score_kernel    score[b] = mean of seg[b, 0 .. S): lane t adds s = t, t + 256, ... in float64, then a fixed tree.
//   si_sdr_kernel        one workgroup of 1,024 lanes per utterance, three passes (means; <x, x> and <x, y>; the residual),
//                        each lane adding i = t, t + 1024, ... in float64, then the tree of vc_speech_gain_f32.
//
// float32 without contraction in the band and segment kernels (tests/stoi_ref.py has their float32 twins).  No atomics, no
// memset, no allocation, no host wait; every count is clamped when it is read; every index taken from memory is checked
// against the buffer before it is used.
#include <cmath>
#include "vc_common.h"

namespace {

constexpr int SW = 256;                 // frame
constexpr int SH = 128;                 // hop
constexpr int SNFFT = 512;
constexpr int SN = 30;                  // frames per segment
constexpr int MAX_FRAMES = 16384;       // 1,024 lanes x 16 frames: the limit of vc_activity_mask / vc_mask_compact too
constexpr int MAX_BANDS = 32;           // one lane of a 32-lane group per band
constexpr int MAX_SAMPLES = 1 << 30;
constexpr int NT = 256;
constexpr int NT_U = 1024;
constexpr int E_TILE = 16;              // frames per workgroup of the energy kernel
constexpr int B_TILE = 4;               // frames per workgroup of the band kernel: one per wave
constexpr int S_TILE = 8;               // segments per workgroup of the segment kernel
constexpr float S_EPS = 2.220446049250313e-16f;                     // 2^-52
constexpr float S_CLIP = 6.623413251903491f;                        // 1 + 10^(15 / 20)

__device__ __forceinline__ int stoi_frames(int len) { return len <= SW ? 0 : (len - SW + SH - 1) / SH; }

// hanning(W + 2)[1 : -1]
__device__ __forceinline__ float stoi_window(int n) { return (float)(0.5 - 0.5 * cospi(2.0 * (double)(n + 1) / (double)(SW + 1))); }

__global__ void __launch_bounds__(NT)
stoi_energy_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, int max_len, int ld,
                   float* __restrict__ energy, int32_t* __restrict__ n_frames, int max_frames) {
#pragma clang fp contract(off)
    __shared__ float w[SW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.y;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    const int F = min(stoi_frames(len), max_frames);
    if (blockIdx.x == 0 && t == 0) n_frames[b] = F;
    w[t] = stoi_window(t);
    __syncthreads();
    const float* __restrict__ x = wav + (size_t)b * ld;
    float* __restrict__ out = energy + (size_t)b * max_frames;
    const int f_end = min((int)(blockIdx.x + 1) * E_TILE, max_frames);
    for (int f = blockIdx.x * E_TILE + wave; f < f_end; f += NT / 64) {        // uniform over the wave
        float v = 0.0f;
        if (f < F) {                                                            // f H + W < len
            const float* a = x + (size_t)f * SH;
#pragma unroll
            for (int i = 0; i < SW / 64; ++i) {
                const float p = a[lane + 64 * i] * w[lane + 64 * i];
                v = v + p * p;
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        }
        if (lane == 0) out[f] = v;
    }
}

__global__ void __launch_bounds__(NT_U)
stoi_keep_kernel(const float* __restrict__ energy, const int32_t* __restrict__ n_frames, int max_frames, float ratio,
                 int32_t* __restrict__ index, int32_t* __restrict__ n_kept) {
#pragma clang fp contract(off)
    __shared__ int sa[NT_U];
    __shared__ float red[NT_U / 64];
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    const int F = min(max(n_frames[b], 0), max_frames);
    const int C = (F + NT_U - 1) / NT_U;
    const float* __restrict__ E = energy + (size_t)b * max_frames;
    float mx = 0.0f;                                                // sums of squares: none is below zero
    for (int f = t; f < F; f += NT_U) mx = fmaxf(mx, E[f]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int v = 1; v < NT_U / 64; ++v) mx = fmaxf(mx, red[v]);
    const float thr = ratio * mx;
    const int c0 = min(t * C, F), c1 = min(c0 + C, F);
    int cnt = 0;
    for (int f = c0; f < c1; ++f) cnt += E[f] > thr ? 1 : 0;
    sa[t] = cnt;
    __syncthreads();
    for (int s = 1; s < NT_U; s <<= 1) {
        const int v = t >= s ? sa[t - s] : 0;
        __syncthreads();
        sa[t] += v;
        __syncthreads();
    }
    const int K = sa[NT_U - 1];
    int32_t* __restrict__ idx = index + (size_t)b * max_frames;
    int k = sa[t] - cnt;
    for (int f = c0; f < c1; ++f)
        if (E[f] > thr) idx[k++] = f;
    for (int f = K + t; f < max_frames; f += NT_U) idx[f] = -1;
    if (t == 0) n_kept[b] = K;
}

struct BandArgs {
    const float* wav[2];     // reference, processed: [B][ld]
    const int32_t* index;    // [B][max_frames]
    const int32_t* n_kept;   // [B]
    const int32_t* bands;    // [nb][2]
    float* T;                // [2][B][max_m][nb]
    int B, max_len, ld, max_frames, max_m, nb;
};

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
#pragma clang fp contract(off)
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

__global__ void __launch_bounds__(NT)
stoi_bands_kernel(BandArgs a) {
#pragma clang fp contract(off)
    __shared__ float2 buf[B_TILE][2][SNFFT];
    __shared__ float2 tw[SNFFT / 2];
    __shared__ float w[SW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.y, sig = blockIdx.z;
    const int m = blockIdx.x * B_TILE + wave;
    const int nb = a.nb, max_m = a.max_m;
    const int K = min(max(a.n_kept[b], 0), a.max_frames);
    const int M = min(max(K - 1, 0), max_m);
    float* __restrict__ out = a.T + (((size_t)sig * a.B + b) * max_m) * nb;
    if ((int)blockIdx.x * B_TILE >= M) {                            // the whole tile lies beyond the utterance
        const int r0 = blockIdx.x * B_TILE, r1 = min(r0 + B_TILE, max_m);
        for (int e = r0 * nb + t; e < r1 * nb; e += NT) out[e] = 0.0f;
        return;
    }
    {
        double s, c;
        sincospi(-2.0 * (double)t / (double)SNFFT, &s, &c);
        tw[t] = make_float2((float)c, (float)s);
        w[t] = stoi_window(t);
    }
    __syncthreads();
    const bool live = m < M;                                        // uniform over the wave
    const float* __restrict__ x = a.wav[sig] + (size_t)b * a.ld;
    const int32_t* __restrict__ idx = a.index + (size_t)b * a.max_frames;
    // a frame number that the buffer cannot hold (the list was not made by vc_stoi_keep_f32) counts as a frame of zeros
    const int f_lim = a.max_len >= SW ? (a.max_len - SW) / SH : -1; // f <= f_lim: f H + W <= max_len
    int fp = -1, fc = -1, fn = -1;
    if (live) {
        fc = idx[m];
        fn = idx[m + 1];                                            // m + 1 <= K - 1
        if (m > 0) fp = idx[m - 1];
        if (fc < 0 || fc > f_lim) fc = -1;
        if (fn < 0 || fn > f_lim) fn = -1;
        if (fp < 0 || fp > f_lim) fp = -1;
    }
    float2* A = buf[wave][0];
    float2* Bf = buf[wave][1];
    // the gather, both windows and the first stage (s = 1: out[2n] = z, out[2n + 1] = z tw[n])
#pragma unroll
    for (int i = 0; i < SW / 64; ++i) {
        const int n = lane + 64 * i;
        const float cur = fc >= 0 ? w[n] * x[(size_t)fc * SH + n] : 0.0f;
        float z;
        if (n < SH) {
            z = cur;
            if (m > 0) z = (fp >= 0 ? w[n + SH] * x[(size_t)fp * SH + SH + n] : 0.0f) + cur;
        } else {
            z = cur + (fn >= 0 ? w[n - SH] * x[(size_t)fn * SH + n - SH] : 0.0f);
        }
        z = z * w[n];
        const float2 q = tw[n];
        A[2 * n] = make_float2(z, 0.0f);
        A[2 * n + 1] = make_float2(z * q.x, z * q.y);
    }
    __syncthreads();
#pragma unroll
    for (int st = 1; st < 9; ++st) {
        const int s = 1 << st;
        const float2* src = (st & 1) ? A : Bf;
        float2* dst = (st & 1) ? Bf : A;
#pragma unroll
        for (int i = 0; i < SW / 64; ++i) {
            const int j = lane + 64 * i;
            const int q = j & (s - 1), ps = j - q;                  // ps = p s
            const float2 u = src[j], v = src[j + SNFFT / 2];
            const float2 d = make_float2(u.x - v.x, u.y - v.y);
            dst[q + 2 * ps] = make_float2(u.x + v.x, u.y + v.y);
            dst[q + 2 * ps + s] = st == 8 ? d : cmul(d, tw[ps]);
        }
        __syncthreads();
    }
    // the result is in A (stage 8 wrote it); |X[k]|^2 for k <= 256 goes to the other buffer
    float* P = reinterpret_cast<float*>(Bf);
    for (int k = lane; k <= SNFFT / 2; k += 64) {
        const float2 v = A[k];
        P[k] = v.x * v.x + v.y * v.y;
    }
    __syncthreads();
    if (m < max_m) {
        for (int j = lane; j < nb; j += 64) {
            const int lo = min(max(a.bands[2 * j], 0), SNFFT / 2 + 1);
            const int hi = min(max(a.bands[2 * j + 1], lo), SNFFT / 2 + 1);
            float acc = 0.0f;
            for (int k = lo; k < hi; ++k) acc = acc + P[k];
            out[(size_t)m * nb + j] = live ? sqrtf(acc) : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(NT)
stoi_seg_kernel(const float* __restrict__ T, const int32_t* __restrict__ n_kept, int B, int max_frames, int max_m, int nb, int mode,
                float* __restrict__ seg, int max_seg) {
#pragma clang fp contract(off)
    __shared__ float Ts[2][S_TILE + SN - 1][MAX_BANDS];
    __shared__ float st[S_TILE][MAX_BANDS][4];
    __shared__ float part[S_TILE][MAX_BANDS];
    const int t = threadIdx.x, g = t >> 5, l = t & 31;
    const int b = blockIdx.y;
    const int s0 = blockIdx.x * S_TILE, s = s0 + g;
    const int K = min(max(n_kept[b], 0), max_frames);
    const int M = min(max(K - 1, 0), max_m);
    const int S = min(max(M - SN + 1, 0), max_seg);
    float* __restrict__ out = seg + (size_t)b * max_seg;
    if (s0 >= S) {                                                  // uniform over the workgroup
        if (l == 0 && s < max_seg) out[s] = 0.0f;
        return;
    }
    for (int e = t; e < 2 * (S_TILE + SN - 1) * MAX_BANDS; e += NT) {
        const int j = e & (MAX_BANDS - 1), r = (e / MAX_BANDS) % (S_TILE + SN - 1), sig = e / (MAX_BANDS * (S_TILE + SN - 1));
        const int row = s0 + r;
        Ts[sig][r][j] = (j < nb && row < M) ? T[(((size_t)sig * B + b) * max_m + row) * nb + j] : 0.0f;
    }
    __syncthreads();
    const bool live = s < S;
    if (mode == 0) {
        float d = 0.0f;
        if (live && l < nb) {
            float sx = 0.0f, sy = 0.0f;
            for (int n = 0; n < SN; ++n) {
                const float x = Ts[0][g + n][l], y = Ts[1][g + n][l];
                sx = sx + x * x;
                sy = sy + y * y;
            }
            const float al = sqrtf(sx) / (sqrtf(sy) + S_EPS);
            float mx = 0.0f, my = 0.0f;
            for (int n = 0; n < SN; ++n) {
                const float x = Ts[0][g + n][l], y = fminf(al * Ts[1][g + n][l], S_CLIP * x);
                mx = mx + x;
                my = my + y;
            }
            mx = mx / (float)SN;
            my = my / (float)SN;
            float qx = 0.0f, qy = 0.0f;
            for (int n = 0; n < SN; ++n) {
                const float x = Ts[0][g + n][l], y = fminf(al * Ts[1][g + n][l], S_CLIP * x);
                const float xc = x - mx, yc = y - my;
                qx = qx + xc * xc;
                qy = qy + yc * yc;
            }
            const float dx = sqrtf(qx) + S_EPS, dy = sqrtf(qy) + S_EPS;
            for (int n = 0; n < SN; ++n) {
                const float x = Ts[0][g + n][l], y = fminf(al * Ts[1][g + n][l], S_CLIP * x);
                d = d + ((x - mx) / dx) * ((y - my) / dy);
            }
        }
        part[g][l] = d;
        __syncthreads();
        if (l == 0 && s < max_seg) {
            float acc = 0.0f;
            if (live) {
                for (int j = 0; j < nb; ++j) acc = acc + part[g][j];
                acc = acc / (float)nb;
            }
            out[s] = acc;
        }
    } else {
        if (live && l < nb) {
            float mx = 0.0f, my = 0.0f;
            for (int n = 0; n < SN; ++n) {
                mx = mx + Ts[0][g + n][l];
                my = my + Ts[1][g + n][l];
            }
            mx = mx / (float)SN;
            my = my / (float)SN;
            float qx = 0.0f, qy = 0.0f;
            for (int n = 0; n < SN; ++n) {
                const float xc = Ts[0][g + n][l] - mx, yc = Ts[1][g + n][l] - my;
                qx = qx + xc * xc;
                qy = qy + yc * yc;
            }
            st[g][l][0] = mx;
            st[g][l][1] = sqrtf(qx) + S_EPS;
            st[g][l][2] = my;
            st[g][l][3] = sqrtf(qy) + S_EPS;
        }
        __syncthreads();
        float p = 0.0f;
        if (live && l < SN) {
            const int n = l;
            float ax = 0.0f, ay = 0.0f;
            for (int j = 0; j < nb; ++j) {
                ax = ax + (Ts[0][g + n][j] - st[g][j][0]) / st[g][j][1];
                ay = ay + (Ts[1][g + n][j] - st[g][j][2]) / st[g][j][3];
            }
            ax = ax / (float)nb;
            ay = ay / (float)nb;
            float qx = 0.0f, qy = 0.0f;
            for (int j = 0; j < nb; ++j) {
                const float xc = (Ts[0][g + n][j] - st[g][j][0]) / st[g][j][1] - ax;
                const float yc = (Ts[1][g + n][j] - st[g][j][2]) / st[g][j][3] - ay;
                qx = qx + xc * xc;
                qy = qy + yc * yc;
            }
            const float dx = sqrtf(qx) + S_EPS, dy = sqrtf(qy) + S_EPS;
            for (int j = 0; j < nb; ++j) {
                const float xc = (Ts[0][g + n][j] - st[g][j][0]) / st[g][j][1] - ax;
                const float yc = (Ts[1][g + n][j] - st[g][j][2]) / st[g][j][3] - ay;
                p = p + (xc / dx) * (yc / dy);
            }
        }
        part[g][l] = p;
        __syncthreads();
        if (l == 0 && s < max_seg) {
            float acc = 0.0f;
            if (live) {
                for (int n = 0; n < SN; ++n) acc = acc + part[g][n];
                acc = acc / (float)SN;
            }
            out[s] = acc;
        }
    }
}

__global__ void __launch_bounds__(NT)
stoi_score_kernel(const float* __restrict__ seg, const int32_t* __restrict__ n_kept, int max_frames, int max_m, int max_seg,
                  float* __restrict__ score, int32_t* __restrict__ n_segments) {
    __shared__ double ss[NT];
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    const int K = min(max(n_kept[b], 0), max_frames);
    const int M = min(max(K - 1, 0), max_m);
    const int S = min(max(M - SN + 1, 0), max_seg);
    const float* __restrict__ in = seg + (size_t)b * max_seg;
    double v = 0.0;
    for (int s = t; s < S; s += NT) v += (double)in[s];
    ss[t] = v;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) ss[t] += ss[t + h];
        __syncthreads();
    }
    if (t == 0) {
        score[b] = S > 0 ? (float)(ss[0] / (double)S) : 0.0f;
        n_segments[b] = S;
    }
}

// the sum of the 1,024 lanes' values: the same tree in every call; every lane returns it
__device__ inline double tree_sum(double v, double* ss) {
    const int t = threadIdx.x;
    __syncthreads();                                                // the previous sum has been read
    ss[t] = v;
    __syncthreads();
    for (int h = NT_U / 2; h > 0; h >>= 1) {
        if (t < h) ss[t] += ss[t + h];
        __syncthreads();
    }
    return ss[0];
}

__global__ void __launch_bounds__(NT_U)
si_sdr_kernel(const float* __restrict__ ref, const float* __restrict__ deg, const int32_t* __restrict__ lens, int max_len, int ld,
              int zero_mean, float* __restrict__ si_sdr, uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)                                      // alpha x - y as a product and a difference, each rounded
    __shared__ double ss[NT_U];
    const int t = threadIdx.x;
    const int b = blockIdx.x;
    const int len = lens ? min(max(lens[b], 0), max_len) : max_len;
    const float* __restrict__ x = ref + (size_t)b * ld;
    const float* __restrict__ y = deg + (size_t)b * ld;
    double mx = 0.0, my = 0.0;
    if (zero_mean && len > 0) {
        double sx = 0.0, sy = 0.0;
        for (int i = t; i < len; i += NT_U) { sx += (double)x[i]; sy += (double)y[i]; }
        mx = tree_sum(sx, ss) / (double)len;
        my = tree_sum(sy, ss) / (double)len;
    }
    double sxx = 0.0, sxy = 0.0;
    for (int i = t; i < len; i += NT_U) {
        const double u = (double)x[i] - mx, v = (double)y[i] - my;
        sxx += u * u;
        sxy += u * v;
    }
    sxx = tree_sum(sxx, ss);
    sxy = tree_sum(sxy, ss);
    const bool ok = len > 0 && sxx > 0.0;                           // uniform over the workgroup
    const double alpha = ok ? sxy / sxx : 0.0;
    double r = 0.0;
    for (int i = t; i < len; i += NT_U) {
        const double e = alpha * ((double)x[i] - mx) - ((double)y[i] - my);
        r += e * e;
    }
    r = tree_sum(r, ss);
    if (t == 0) {
        float v = 0.0f;
        if (ok) {
            const double num = alpha * alpha * sxx;
            if (num == 0.0) v = -INFINITY;                          // nothing of the reference in y
            else if (r == 0.0) v = INFINITY;                        // alpha x - y vanishes exactly: y == x
            else v = (float)(10.0 * log10(num / r));
        }
        si_sdr[b] = v;
        valid[b] = ok ? 1 : 0;
    }
}

inline int frames_of(int len) { return len <= SW ? 0 : (len - SW + SH - 1) / SH; }

}  // namespace

extern "C" {

int vc_stoi_energy_f32(const float* d_ref, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld, float* d_energy,
                       int32_t* d_n_frames, int32_t max_frames, void* stream) {
    const char* fn = "vc_stoi_energy_f32";
    VC_REQUIRE(d_ref && d_energy && d_n_frames, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_len >= 1 && max_len <= MAX_SAMPLES && ld >= max_len,
               "%s: bad shape (batch %d in [1, 65535], max_len %d in [1, %d], ld %d >= max_len)", fn, batch, max_len, MAX_SAMPLES, ld);
    VC_REQUIRE(max_frames >= 1 && max_frames <= MAX_FRAMES && max_frames >= frames_of(max_len),
               "%s: max_frames %d must lie in [1, %d] and hold the %d frames of max_len %d", fn, max_frames, MAX_FRAMES,
               frames_of(max_len), max_len);
    const dim3 grid((unsigned)((max_frames + E_TILE - 1) / E_TILE), (unsigned)batch);
    hipLaunchKernelGGL(stoi_energy_kernel, grid, dim3(NT), 0, static_cast<hipStream_t>(stream), d_ref, d_lens, max_len, ld, d_energy,
                       d_n_frames, max_frames);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_stoi_keep_f32(const float* d_energy, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float ratio,
                     int32_t* d_index, int32_t* d_n_kept, void* stream) {
    const char* fn = "vc_stoi_keep_f32";
    VC_REQUIRE(d_energy && d_n_frames && d_index && d_n_kept, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && max_frames <= MAX_FRAMES,
               "%s: bad shape (batch %d in [1, 65535], max_frames %d in [1, %d])", fn, batch, max_frames, MAX_FRAMES);
    VC_REQUIRE(std::isfinite(ratio) && ratio > 0.0f && ratio < 1.0f, "%s: the ratio 10^(-dyn / 10) must lie in (0, 1), got %g", fn,
               (double)ratio);
    hipLaunchKernelGGL(stoi_keep_kernel, dim3(batch), dim3(NT_U), 0, static_cast<hipStream_t>(stream), d_energy, d_n_frames, max_frames,
                       ratio, d_index, d_n_kept);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_stoi_bands_f32(const float* d_ref, const float* d_deg, int32_t batch, int32_t max_len, int32_t ld, const int32_t* d_index,
                      const int32_t* d_n_kept, int32_t max_frames, const int32_t* d_bands, int32_t n_bands, float* d_T, int32_t max_m,
                      void* stream) {
    const char* fn = "vc_stoi_bands_f32";
    VC_REQUIRE(d_ref && d_deg && d_index && d_n_kept && d_bands && d_T, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_len >= 1 && max_len <= MAX_SAMPLES && ld >= max_len,
               "%s: bad shape (batch %d in [1, 65535], max_len %d in [1, %d], ld %d >= max_len)", fn, batch, max_len, MAX_SAMPLES, ld);
    VC_REQUIRE(max_frames >= 1 && max_frames <= MAX_FRAMES && max_m >= 1 && max_m <= MAX_FRAMES,
               "%s: max_frames %d and max_m %d must lie in [1, %d]", fn, max_frames, max_m, MAX_FRAMES);
    VC_REQUIRE(n_bands >= 1 && n_bands <= MAX_BANDS, "%s: n_bands %d must lie in [1, %d]", fn, n_bands, MAX_BANDS);
    BandArgs a;
    a.wav[0] = d_ref; a.wav[1] = d_deg; a.index = d_index; a.n_kept = d_n_kept; a.bands = d_bands; a.T = d_T;
    a.B = batch; a.max_len = max_len; a.ld = ld; a.max_frames = max_frames; a.max_m = max_m; a.nb = n_bands;
    const dim3 grid((unsigned)((max_m + B_TILE - 1) / B_TILE), (unsigned)batch, 2);
    hipLaunchKernelGGL(stoi_bands_kernel, grid, dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_stoi_score_f32(const float* d_T, const int32_t* d_n_kept, int32_t batch, int32_t max_frames, int32_t max_m, int32_t n_bands,
                      int32_t mode, float* d_seg, int32_t max_seg, float* d_score, int32_t* d_n_segments, void* stream) {
    const char* fn = "vc_stoi_score_f32";
    VC_REQUIRE(d_T && d_n_kept && d_seg && d_score && d_n_segments, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && max_frames <= MAX_FRAMES && max_m >= 1 && max_m <= MAX_FRAMES &&
               max_seg >= 1 && max_seg <= MAX_FRAMES,
               "%s: bad shape (batch %d in [1, 65535]; max_frames %d, max_m %d, max_seg %d in [1, %d])", fn, batch, max_frames, max_m,
               max_seg, MAX_FRAMES);
    VC_REQUIRE(n_bands >= 1 && n_bands <= MAX_BANDS, "%s: n_bands %d must lie in [1, %d]", fn, n_bands, MAX_BANDS);
    VC_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (STOI) or 1 (ESTOI), got %d", fn, mode);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((max_seg + S_TILE - 1) / S_TILE), (unsigned)batch);
    hipLaunchKernelGGL(stoi_seg_kernel, grid, dim3(NT), 0, st, d_T, d_n_kept, batch, max_frames, max_m, n_bands, mode, d_seg, max_seg);
    VC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(stoi_score_kernel, dim3(batch), dim3(NT), 0, st, d_seg, d_n_kept, max_frames, max_m, max_seg, d_score,
                       d_n_segments);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_si_sdr_f32(const float* d_ref, const float* d_deg, const int32_t* d_lens, int32_t batch, int32_t max_len, int32_t ld,
                  int32_t zero_mean, float* d_si_sdr, uint8_t* d_valid, void* stream) {
    const char* fn = "vc_si_sdr_f32";
    VC_REQUIRE(d_ref && d_deg && d_si_sdr && d_valid, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_len >= 1 && max_len <= MAX_SAMPLES && ld >= max_len,
               "%s: bad shape (batch %d in [1, 65535], max_len %d in [1, %d], ld %d >= max_len)", fn, batch, max_len, MAX_SAMPLES, ld);
    VC_REQUIRE(zero_mean == 0 || zero_mean == 1, "%s: zero_mean must be 0 or 1, got %d", fn, zero_mean);
    hipLaunchKernelGGL(si_sdr_kernel, dim3(batch), dim3(NT_U), 0, static_cast<hipStream_t>(stream), d_ref, d_deg, d_lens, max_len, ld,
                       zero_mean, d_si_sdr, d_valid);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
