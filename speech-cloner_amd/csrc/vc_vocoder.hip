// Griffin-Lim vocoder for gfx950: magnitude spectrogram -> waveform.
//
// Replaces /root/reference/audio_lib.py:249-308 (griffin_lim_alg, from_power_to_wav) and :31-47
// (calc_inv_preemphasis), which loop librosa.istft / librosa.stft on the CPU.
//
// One iteration of the reference is  wav = istft(S);  S' = amp * phase(stft(wav)).  Here the state
// between iterations is the set of windowed synthesis frames  y_f[n] = w[n] * irfft(S_f)[n]
// ([frames, n_fft] float32, ping-pong), and ONE kernel per iteration does, per tile of 16 frames:
//   gather   the overlap-add of the previous frames at the samples this tile's analysis windows
//            cover, divided by the window sum-square (librosa.istft), with librosa.stft's reflect
//            padding folded into the index,
//   forward  400-point real DFT (25 x 16 split of fe_dft400.h),
//   project  S = amp * Z / |Z|  (phase of a zero bin is 0),
//   inverse  16-point inverse DFTs + hermitian 25-point inverse, synthesis window, store.
// The thread that finishes bin group k1 of the forward transform holds exactly the 16 bins
// S[k1 + 25 k2] the inverse needs, so the spectrum never leaves registers.
// The kernel is bound by LDS traffic and launch latency (a 1000-frame utterance is 63 blocks);
// HBM sees 2 x frames x n_fft x 4 bytes per iteration, all L2-resident.
//
// Fast Griffin-Lim (Perraudin, Balazs & Sondergaard 2013; librosa's formulation): the projection
// takes the phase of  C_i = R_i - beta R_{i-1}  instead of R_i = stft(istft(S_{i-1})), with
// beta = momentum / (1 + momentum).  The kernels carry R between iterations in a per-frame state
// (MOM template flavours); the first projection sees R_0 = 0 and never reads the state.
#include <cmath>
#include <cstring>
#include <vector>
#include "vc_device.h"
#include "fe_dft400.h"

namespace {

constexpr int VT = 256;            // threads per block
constexpr int VG = 16;             // frames per block (400-point path)
constexpr int VGG = 4;             // frames per block (generic path)
constexpr int VA_STRIDE = 17;
constexpr float F32_TINY = 1.17549435e-38f;
constexpr int NSLOT400 = 13 * 16;  // momentum state slots per frame (400-point path): [k1][k2]

// Momentum flavour of an iteration kernel.  MOM_OFF is the plain algorithm (the only flavour
// vc_griffin_lim_f32 launches); MOM_FIRST stores R_1 and projects it unchanged (R_0 = 0);
// MOM_ON reads R_{i-1}, projects C_i = R_i - beta R_{i-1}, stores R_i in place.
enum : int { MOM_OFF = 0, MOM_FIRST = 1, MOM_ON = 2 };

struct GlArgs {
    const float* amp;        // [B][maxF][nb]
    const float* phase0;     // [B][maxF][nb]  (init kernel only)
    const float* prev;       // [B][maxF][N]
    float* next;             // [B][maxF][N]
    const int32_t* n_frames; // [B] or null
    const float* window;     // [N] | tw400[416] | twg[2N]
    int maxF, nb, N, hop, span, nov;
    float2* mom;             // R_{i-1}: [B][maxF][13][16] (400-point slot order) | [B][maxF][nb]; MOM != MOM_OFF only
    float beta;              // momentum / (1 + momentum)
};

__device__ __forceinline__ int utt_frames(const GlArgs& a, int b) {
    return a.n_frames ? min(max(a.n_frames[b], 0), a.maxF) : a.maxF;
}

__device__ __forceinline__ void copy_lds(float* dst, const float* src, int n) {
    for (int i = threadIdx.x; i < n; i += VT) dst[i] = src[i];
}

// Overlap-add of the stored frames at untrimmed position q of utterance frames `fr` ([F][N]),
// normalised like librosa.istft.  win = padded window (LDS).
__device__ __forceinline__ float ola_at(const float* fr, const float* win, int q, int F, int N, int hop, int nov) {
    const int fhi = min(q / hop, F - 1);
    float acc = 0.0f, wss = 0.0f;
#pragma unroll 5
    for (int j = 0; j < nov; ++j) {
        const int f = fhi - j;
        const int o = q - f * hop;
        const bool ok = (f >= 0) && (o < N);
        const int fc = max(f, 0), oc = min(o, N - 1);
        const float v = fr[(size_t)fc * N + oc];
        const float w = win[oc];
        acc += ok ? v : 0.0f;
        wss += ok ? w * w : 0.0f;
    }
    return wss > F32_TINY ? acc / wss : acc;
}

// Samples of the reflect-padded, trimmed signal this tile needs -> xs[0..span)
__device__ __forceinline__ void gather_tile(const GlArgs& a, const float* fr, const float* win, int F, int f0, float* xs) {
    const int half = a.N / 2;
    const int L = a.hop * (F - 1);
    for (int i = threadIdx.x; i < a.span; i += VT) {
        const int p = f0 * a.hop + i;                 // position in the padded signal
        float v = 0.0f;
        if (p < L + a.N) {
            int n = p - half;
            n = n < 0 ? -n : (n >= L ? 2 * (L - 1) - n : n);
            n = min(max(n, 0), L - 1);
            v = ola_at(fr, win, n + half, F, a.N, a.hop, a.nov);
        }
        xs[i] = v;
    }
}

// ---- the transform halves every STFT-domain kernel below is made of: one definition each, its roundings written down
// (explicit fmaf, nothing left to contract: fe_dft400.h "pinned forms"), the same bits in every caller.
// LDS of a 400-point tile: the plan's window [400] and twiddles [2][208], the transform's rows Are, Aim [NROW][VA_STRIDE], then
// the kernel's own (the gathered samples [span]; INIT: the magnitude and the phase tile)
constexpr int NROW = VG * 13;
struct Tile400 { float *win, *tw, *Are, *Aim, *rest; };
__device__ __forceinline__ Tile400 carve400(char* smem) {
    float* win = reinterpret_cast<float*>(smem);
    return {win, win + 400, win + 816, win + 816 + NROW * VA_STRIDE, win + 816 + 2 * NROW * VA_STRIDE};
}

// Thread (g, k1) = tid / 13, tid % 13 holds the 16 slots S[k1 + 25 k2] of frame g.  Their values from rows [VG][201] of
// per-bin magnitudes or gains (a conjugate slot: the value of its mirror bin); 0 in a thread without a live frame.
__device__ __forceinline__ void load_slots400(const float* rows, int nvalid, int tid, float* v) {
    const int g = min(tid / 13, VG - 1), k1 = tid - (tid / 13) * 13;
    const bool live = tid < NROW && g < nvalid;
    const float* src = rows + (size_t)(live ? g : 0) * 201;
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        bool cj;
        const int bin = vcfe::src_bin(live ? k1 : 0, k2, cj);
        const float x = src[bin];
        v[k2] = live ? x : 0.0f;
    }
}

// Forward steps 1 and 2, thread (g, n2): frame g of the samples xs, windowed -> A[k1][n2] W400^(n2 k1); TW: vcfe::pinned::twiddle400
template <unsigned TW>
__device__ __forceinline__ void forward400_rows(const Tile400& t, const float* xs, int hop, int tid) {
    const int g = tid >> 4, n2 = tid & 15;
    const float* xp = xs + g * hop + n2;
    float x[25], w[25], ar[13], ai[13];
#pragma unroll
    for (int n1 = 0; n1 < 25; ++n1) { x[n1] = xp[16 * n1]; w[n1] = t.win[16 * n1 + n2]; }
    vcfe::pinned::rdft25_13_win(x, w, ar, ai);
    const int i0 = VA_STRIDE * (g * 13) + n2;
#pragma unroll
    for (int k1 = 0; k1 < 13; ++k1) {
        vcfe::pinned::twiddle400<TW>(ar[k1], ai[k1], t.tw[k1 * 16 + n2], t.tw[208 + k1 * 16 + n2], k1);
        t.Are[i0 + VA_STRIDE * k1] = ar[k1];
        t.Aim[i0 + VA_STRIDE * k1] = ai[k1];
    }
}

// Forward step 3, row tid < NROW: its 16 slots are the bins k1 + 25 k2 and the conjugates of the mirrors of those above 200
__device__ __forceinline__ void forward400_cols(const Tile400& t, int tid, float* yr, float* yi) {
    float zr[16], zi[16];
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) { zr[n2] = t.Are[VA_STRIDE * tid + n2]; zi[n2] = t.Aim[VA_STRIDE * tid + n2]; }
    vcfe::pinned::cdft16(zr, zi, yr, yi);
}

// the 16 slots zr / zi of row tid < NROW: inverse 16-point stage, conjugate twiddle -> B[k1][n2] in A's place
__device__ __forceinline__ void inverse400_cols(float* zr, float* zi, const float* tw, float* Are, float* Aim, int tid, int k1) {
    float yr[16], yi[16];
    vcfe::cidft16(zr, zi, yr, yi);
#pragma unroll
    for (int n2 = 0; n2 < 16; ++n2) {
        vcfe::cmul(yr[n2], yi[n2], tw[k1 * 16 + n2], -tw[208 + k1 * 16 + n2]);
        Are[VA_STRIDE * tid + n2] = yr[n2];
        Aim[VA_STRIDE * tid + n2] = yi[n2];
    }
}

// thread (g, n2), g < nvalid: hermitian 25-point inverse, synthesis window, store the frame; tile: the first frame's [400]
__device__ __forceinline__ void inverse400_rows(const float* Are, const float* Aim, const float* win, float* tile, int nvalid,
                                                int tid) {
    const int g = tid >> 4, n2 = tid & 15;
    if (g < nvalid) {
        float br[13], bi[13], x[25];
        const int i0 = VA_STRIDE * (g * 13) + n2;
#pragma unroll
        for (int k1 = 0; k1 < 13; ++k1) { br[k1] = Are[i0 + VA_STRIDE * k1]; bi[k1] = Aim[i0 + VA_STRIDE * k1]; }
        vcfe::hdft25_real(br, bi, x);
        float* out = tile + (size_t)g * 400 + n2;
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) out[16 * n1] = x[n1] * win[16 * n1 + n2] * (1.0f / 400.0f);
    }
}

// LDS of a generic-path tile: the plan's window [N] and twiddle table twr, twi [N] each, then the kernel's own
struct TileGen { float *win, *twr, *twi, *rest; };
__device__ __forceinline__ TileGen carve_generic(char* smem, int N) {
    float* win = reinterpret_cast<float*>(smem);
    return {win, win + N, win + 2 * N, win + 3 * N};
}
__device__ __forceinline__ void load_generic(const TileGen& t, const float* tables, int N) {
    copy_lds(t.win, tables, N);
    copy_lds(t.twr, tables + N + 416, 2 * N);
}

// The generic path's two sums.  Bin k of the frame at xp: sum_n (x[n] w[n]) exp(-2 pi i k n / N)
__device__ __forceinline__ void forward_generic_bin(const float* xp, const float* win, const float* twr, const float* twi, int k,
                                                    int N, float& re, float& im) {
    re = 0.0f; im = 0.0f;
    int m = 0;
    for (int n = 0; n < N; ++n) {
        const float xv = xp[n] * win[n];
        re = fmaf(xv, twr[m], re);
        im = fmaf(xv, twi[m], im);
        m += k; if (m >= N) m -= N;
    }
}

// Sample n of the windowed inverse of sr / si [nb] (Im of bin 0 and bin N / 2 not read), twr = cos, twi = -sin:
// x[n] = (1/N) [S0 + (-1)^n S_{N/2} + 2 sum_{k=1}^{N/2-1} (Sr cos(2 pi k n/N) - Si sin(2 pi k n/N))]
__device__ __forceinline__ float inverse_generic_sample(const float* sr, const float* si, const float* win, const float* twr,
                                                        const float* twi, int n, int N, int nb, float invN) {
    float acc = 0.0f;
    int m = n;                                        // (k n) mod N for k = 1
    for (int k = 1; k < nb - 1; ++k) {
        acc = fmaf(sr[k], twr[m], acc);
        acc = fmaf(si[k], twi[m], acc);
        m += n; if (m >= N) m -= N;
    }
    const float edge = sr[0] + ((n & 1) ? -sr[nb - 1] : sr[nb - 1]);
    return (edge + 2.0f * acc) * invN * win[n];
}

// 400-point iteration (INIT: spectrum = amp * exp(i phase0) instead of the analysis of prev).
template <bool INIT, int MOM>
__global__ void __launch_bounds__(VT)
gl_iter400_kernel(GlArgs a) {
    static_assert(!INIT || MOM == MOM_OFF, "the initial spectrum has no momentum");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Tile400 t = carve400(smem);
    float *win = t.win, *tw = t.tw, *Are = t.Are, *Aim = t.Aim;
    // INIT keeps the magnitude tile and the phase tile in LDS; the iteration kernel holds each
    // thread's 16 target magnitudes in registers instead (38 KB of LDS: four blocks per CU)
    float* amps = t.rest;    // INIT: [VG][201]
    float* xs = INIT ? amps + VG * 201 : amps;         // [span]  (INIT: phase tile [VG][201])

    const int b = blockIdx.y, tid = threadIdx.x;
    const int F = utt_frames(a, b);
    const int f0 = blockIdx.x * VG;
    if (f0 >= F) return;
    const int nvalid = min(VG, F - f0);

    copy_lds(win, a.window, 816);
    float amr[16];
    if constexpr (INIT) {
        const float* src = a.amp + ((size_t)b * a.maxF + f0) * 201;
        for (int i = tid; i < VG * 201; i += VT) amps[i] = (i < nvalid * 201) ? src[i] : 0.0f;
        const float* ps = a.phase0 + ((size_t)b * a.maxF + f0) * 201;
        for (int i = tid; i < VG * 201; i += VT) xs[i] = (i < nvalid * 201) ? ps[i] : 0.0f;
    } else {
        load_slots400(a.amp + ((size_t)b * a.maxF + f0) * 201, nvalid, tid, amr);
    }
    __syncthreads();
    if (!INIT) {
        gather_tile(a, a.prev + (size_t)b * a.maxF * 400, win, F, f0, xs);
        __syncthreads();
        forward400_rows<vcfe::pinned::TW_FILTER>(t, xs, a.hop, tid);
        __syncthreads();
    }
    // thread (g, k1): forward 16-point stage, projection onto the target magnitude, inverse
    // 16-point stage, conjugate twiddle -> B[k1][n2].  In line, here and in stft_filter400_kernel: the products of the
    // projection (am * ur, gr * yr) are fused into the first additions of cidft16, and the cdft16 before them was compiled
    // to other choices than vcfe::pinned::cdft16 holds (one of its eight twiddles); these two kernels keep their bits.
    if (tid < NROW) {
        const int g = tid / 13, k1 = tid - g * 13;
        float zr[16], zi[16], yr[16], yi[16];
        if (!INIT) {
#pragma unroll
            for (int n2 = 0; n2 < 16; ++n2) { zr[n2] = Are[VA_STRIDE * tid + n2]; zi[n2] = Aim[VA_STRIDE * tid + n2]; }
            vcfe::cdft16(zr, zi, yr, yi);
        }
        if constexpr (MOM != MOM_OFF) {
            // this thread's 16 slots of R_i (bins k1 + 25 k2, conjugate copies included) are its own:
            // read R_{i-1}, store R_i in place (128 contiguous bytes), project C = R_i - beta R_{i-1}
            if (g < nvalid) {
                float4* st = reinterpret_cast<float4*>(a.mom + (((size_t)b * a.maxF + f0 + g) * 13 + k1) * 16);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float4 r = make_float4(yr[2 * j], yi[2 * j], yr[2 * j + 1], yi[2 * j + 1]);
                    if constexpr (MOM == MOM_ON) {
                        const float4 q = st[j];
                        yr[2 * j] = fmaf(-a.beta, q.x, r.x);
                        yi[2 * j] = fmaf(-a.beta, q.y, r.y);
                        yr[2 * j + 1] = fmaf(-a.beta, q.z, r.z);
                        yi[2 * j + 1] = fmaf(-a.beta, q.w, r.w);
                    }
                    st[j] = r;
                }
            }
        }
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            bool cj;
            const int bin = vcfe::src_bin(k1, k2, cj);
            const float am = INIT ? amps[g * 201 + bin] : amr[k2];
            float ur, ui;
            if (INIT) {
                float s, c;
                sincosf(xs[g * 201 + bin], &s, &c);
                ur = c; ui = cj ? -s : s;
            } else {
                const float m2 = yr[k2] * yr[k2] + yi[k2] * yi[k2];
                const float inv = m2 > 0.0f ? rsqrtf(m2) : 0.0f;
                ur = m2 > 0.0f ? yr[k2] * inv : 1.0f;
                ui = yi[k2] * inv;
            }
            zr[k2] = am * ur;
            zi[k2] = am * ui;
        }
        vcfe::cidft16(zr, zi, yr, yi);
#pragma unroll
        for (int n2 = 0; n2 < 16; ++n2) {
            vcfe::cmul(yr[n2], yi[n2], tw[k1 * 16 + n2], -tw[208 + k1 * 16 + n2]);
            Are[VA_STRIDE * tid + n2] = yr[n2];
            Aim[VA_STRIDE * tid + n2] = yi[n2];
        }
    }
    __syncthreads();
    inverse400_rows(Are, Aim, win, a.next + ((size_t)b * a.maxF + f0) * 400, nvalid, tid);
}

// Generic path (any even n_fft): direct O(N^2) DFTs from the LDS twiddle table twg[m] =
// exp(-2 pi i m / N).  VGG frames per block.
template <bool INIT, int MOM>
__global__ void __launch_bounds__(VT)
gl_iter_generic_kernel(GlArgs a) {
    static_assert(!INIT || MOM == MOM_OFF, "the initial spectrum has no momentum");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, nb = a.nb;
    const TileGen t = carve_generic(smem, N);
    float *win = t.win, *twr = t.twr, *twi = t.twi, *Sr = t.rest;    // [VGG][nb]
    float* Si = Sr + VGG * nb;
    float* xs = Si + VGG * nb;                         // [span]

    const int b = blockIdx.y, tid = threadIdx.x;
    const int F = utt_frames(a, b);
    const int f0 = blockIdx.x * VGG;
    if (f0 >= F) return;
    const int nvalid = min(VGG, F - f0);
    load_generic(t, a.window, N);
    __syncthreads();
    if (!INIT) {
        gather_tile(a, a.prev + (size_t)b * a.maxF * N, win, F, f0, xs);
        __syncthreads();
    }
    for (int idx = tid; idx < nvalid * nb; idx += VT) {
        const int g = idx / nb, k = idx - g * nb;
        const float am = a.amp[((size_t)b * a.maxF + f0 + g) * nb + k];
        float ur, ui;
        if (INIT) {
            float s, c;
            sincosf(a.phase0[((size_t)b * a.maxF + f0 + g) * nb + k], &s, &c);
            ur = c; ui = s;
        } else {
            // forward_generic_bin's sum in line: which square of m2 below is fused follows this text, differently per flavour
            const float* xp = xs + g * a.hop;
            float re = 0.0f, im = 0.0f;
            int m = 0;
            for (int n = 0; n < N; ++n) {
                const float xv = xp[n] * win[n];
                re = fmaf(xv, twr[m], re);
                im = fmaf(xv, twi[m], im);
                m += k; if (m >= N) m -= N;
            }
            if constexpr (MOM != MOM_OFF) {
                float2* st = a.mom + ((size_t)b * a.maxF + f0 + g) * nb + k;
                const float2 r = make_float2(re, im);
                if constexpr (MOM == MOM_ON) {
                    const float2 q = *st;
                    re = fmaf(-a.beta, q.x, re);
                    im = fmaf(-a.beta, q.y, im);
                }
                *st = r;
            }
            const float m2 = re * re + im * im;
            const float inv = m2 > 0.0f ? rsqrtf(m2) : 0.0f;
            ur = m2 > 0.0f ? re * inv : 1.0f;
            ui = im * inv;
        }
        Sr[idx] = am * ur;
        Si[idx] = am * ui;
    }
    __syncthreads();
    const float invN = 1.0f / (float)N;
    for (int idx = tid; idx < nvalid * N; idx += VT) {
        const int g = idx / N, n = idx - g * N;
        a.next[((size_t)b * a.maxF + f0 + g) * N + n] =
            inverse_generic_sample(Sr + g * nb, Si + g * nb, win, twr, twi, n, N, nb, invN);
    }
}

// ---- STFT-domain filter (include/vc_hip.h, "Differential-spectrum conversion"): frames of istft(G * stft(x)).
// The iteration kernels with two changes: the gather reads the reflect-padded WAVEFORM (not the overlap-add of stored
// frames), and the projection amp * Z / |Z| is the product G * Z.  Same tiles, same LDS, same transforms.
struct SfArgs {
    const float* wav;        // [B][wav_stride]
    const int32_t* len;      // [B]
    const float* gain;       // [B][maxF][nb]
    const int32_t* n_frames; // [B] or null
    float* frames;           // [B][maxF][N]
    int32_t* f_out;          // [B]: F_b for the overlap-add launch behind this one
    const float* window;     // [N] | tw400[416] | twg[2N]
    int wav_stride, maxF, nb, N, hop, span;
};

// F_b, 0 for an utterance the reflect padding does not fit; len: the clamped sample count.  The first workgroup records F_b.
__device__ __forceinline__ int sf_frames(const SfArgs& a, int b, int& len) {
    len = min(max(a.len[b], 0), a.wav_stride);
    int F = min(a.maxF, 1 + len / a.hop);
    if (a.n_frames) F = min(F, max(a.n_frames[b], 0));
    if (len <= a.N / 2 || a.hop * (F - 1) <= a.N / 2) F = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.f_out[b] = F;
    return F;
}

// Samples of the reflect-padded signal x[0, len) this tile needs -> xs[0..span); len > N / 2, F >= 2
__device__ __forceinline__ void sf_gather_tile(const SfArgs& a, const float* x, int len, int F, int f0, float* xs) {
    const int half = a.N / 2;
    const int end = a.hop * (F - 1) + a.N;                // <= len + N: the padded signal
    for (int i = threadIdx.x; i < a.span; i += VT) {
        const int p = f0 * a.hop + i;
        float v = 0.0f;
        if (p < end) {
            int n = p - half;
            n = n < 0 ? -n : (n >= len ? 2 * (len - 1) - n : n);
            v = x[min(max(n, 0), len - 1)];
        }
        xs[i] = v;
    }
}

__global__ void __launch_bounds__(VT)
stft_filter400_kernel(SfArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Tile400 t = carve400(smem);
    float *win = t.win, *tw = t.tw, *Are = t.Are, *Aim = t.Aim, *xs = t.rest;

    const int b = blockIdx.y, tid = threadIdx.x;
    int len;
    const int F = sf_frames(a, b, len);
    const int f0 = blockIdx.x * VG;
    if (f0 >= F) return;
    const int nvalid = min(VG, F - f0);

    copy_lds(win, a.window, 816);
    float gr[16];                                      // the gains of this thread's 16 slots, as amr[] of the iteration kernel
    load_slots400(a.gain + ((size_t)b * a.maxF + f0) * 201, nvalid, tid, gr);
    __syncthreads();
    sf_gather_tile(a, a.wav + (size_t)b * a.wav_stride, len, F, f0, xs);
    __syncthreads();
    forward400_rows<vcfe::pinned::TW_FILTER>(t, xs, a.hop, tid);
    __syncthreads();
    // thread (g, k1): forward 16-point stage, G * Z, inverse 16-point stage, conjugate twiddle -> B[k1][n2]; in line for
    // the reason given in gl_iter400_kernel
    if (tid < NROW) {
        const int k1 = tid - (tid / 13) * 13;
        float zr[16], zi[16], yr[16], yi[16];
#pragma unroll
        for (int n2 = 0; n2 < 16; ++n2) { zr[n2] = Are[VA_STRIDE * tid + n2]; zi[n2] = Aim[VA_STRIDE * tid + n2]; }
        vcfe::cdft16(zr, zi, yr, yi);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            zr[k2] = gr[k2] * yr[k2];
            zi[k2] = gr[k2] * yi[k2];
        }
        vcfe::cidft16(zr, zi, yr, yi);
#pragma unroll
        for (int n2 = 0; n2 < 16; ++n2) {
            vcfe::cmul(yr[n2], yi[n2], tw[k1 * 16 + n2], -tw[208 + k1 * 16 + n2]);
            Are[VA_STRIDE * tid + n2] = yr[n2];
            Aim[VA_STRIDE * tid + n2] = yi[n2];
        }
    }
    __syncthreads();
    inverse400_rows(Are, Aim, win, a.frames + ((size_t)b * a.maxF + f0) * 400, nvalid, tid);
}

__global__ void __launch_bounds__(VT)
stft_filter_generic_kernel(SfArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, nb = a.nb;
    const TileGen t = carve_generic(smem, N);
    float *win = t.win, *twr = t.twr, *twi = t.twi, *Sr = t.rest;    // [VGG][nb]
    float* Si = Sr + VGG * nb;
    float* xs = Si + VGG * nb;                         // [span]

    const int b = blockIdx.y, tid = threadIdx.x;
    int len;
    const int F = sf_frames(a, b, len);
    const int f0 = blockIdx.x * VGG;
    if (f0 >= F) return;
    const int nvalid = min(VGG, F - f0);
    load_generic(t, a.window, N);
    __syncthreads();
    sf_gather_tile(a, a.wav + (size_t)b * a.wav_stride, len, F, f0, xs);
    __syncthreads();
    for (int idx = tid; idx < nvalid * nb; idx += VT) {
        const int g = idx / nb, k = idx - g * nb;
        const float gn = a.gain[((size_t)b * a.maxF + f0 + g) * nb + k];
        float re, im;
        forward_generic_bin(xs + g * a.hop, win, twr, twi, k, N, re, im);
        Sr[idx] = gn * re;
        Si[idx] = gn * im;
    }
    __syncthreads();
    const float invN = 1.0f / (float)N;
    for (int idx = tid; idx < nvalid * N; idx += VT) {
        const int g = idx / N, n = idx - g * N;
        a.frames[((size_t)b * a.maxF + f0 + g) * N + n] =
            inverse_generic_sample(Sr + g * nb, Si + g * nb, win, twr, twi, n, N, nb, invN);
    }
}

// ---- linear short-time power (include/vc_hip.h, "Noise suppression"): P = |stft(x)|^2 with the filter's framing.  The
// forward half of the filter kernels, then re^2 + im^2 instead of the gain and the inverse half.  A workgroup owns the rows
// of its tile: rows at or beyond F_b are written as 0 here, so the launch needs no memset and writes every element once.
__device__ __forceinline__ void sp_zero_rows(float* dst, int n) {
    for (int i = threadIdx.x; i < n; i += VT) dst[i] = 0.0f;
}

__global__ void __launch_bounds__(VT)
stft_power400_kernel(SfArgs a, float* __restrict__ power) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Tile400 t = carve400(smem);
    float *win = t.win, *Are = t.Are, *xs = t.rest;    // Are: later the tile's power [VG][201]
    static_assert(VG * 201 <= NROW * VA_STRIDE, "the power tile must fit the transform's rows");

    const int b = blockIdx.y, tid = threadIdx.x;
    int len;
    const int F = sf_frames(a, b, len);
    const int f0 = blockIdx.x * VG;
    const int nrows = min(VG, a.maxF - f0);            // rows of d_power this tile owns
    float* dst = power + ((size_t)b * a.maxF + f0) * 201;
    if (f0 >= F) { sp_zero_rows(dst, nrows * 201); return; }
    const int nvalid = min(VG, F - f0);

    copy_lds(win, a.window, 816);
    __syncthreads();
    sf_gather_tile(a, a.wav + (size_t)b * a.wav_stride, len, F, f0, xs);
    __syncthreads();
    forward400_rows<vcfe::pinned::TW_POWER>(t, xs, a.hop, tid);
    __syncthreads();
    float yr[16], yi[16];
    if (tid < NROW) forward400_cols(t, tid, yr, yi);
    __syncthreads();                                   // every row of Are has been read
    if (tid < NROW) {
        const int g = tid / 13, k1 = tid - g * 13;
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            bool cj;
            const int bin = vcfe::src_bin(k1, k2, cj);
            // the mirrors of k1 == 0 are the bins 25, 50, .. 175 again: each bin is stored by one slot
            if (!cj || k1 != 0) Are[g * 201 + bin] = yr[k2] * yr[k2] + yi[k2] * yi[k2];
        }
    }
    __syncthreads();
    for (int i = tid; i < nrows * 201; i += VT) dst[i] = i < nvalid * 201 ? Are[i] : 0.0f;
}

__global__ void __launch_bounds__(VT)
stft_power_generic_kernel(SfArgs a, float* __restrict__ power) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, nb = a.nb;
    const TileGen t = carve_generic(smem, N);
    float *win = t.win, *twr = t.twr, *twi = t.twi, *xs = t.rest;    // [span]

    const int b = blockIdx.y, tid = threadIdx.x;
    int len;
    const int F = sf_frames(a, b, len);
    const int f0 = blockIdx.x * VGG;
    const int nrows = min(VGG, a.maxF - f0);
    float* dst = power + ((size_t)b * a.maxF + f0) * nb;
    if (f0 >= F) { sp_zero_rows(dst, nrows * nb); return; }
    const int nvalid = min(VGG, F - f0);
    load_generic(t, a.window, N);
    __syncthreads();
    sf_gather_tile(a, a.wav + (size_t)b * a.wav_stride, len, F, f0, xs);
    __syncthreads();
    for (int idx = tid; idx < nrows * nb; idx += VT) {
        float re = 0.0f, im = 0.0f;
        if (idx < nvalid * nb) {
            const int g = idx / nb, k = idx - g * nb;
            forward_generic_bin(xs + g * a.hop, win, twr, twi, k, N, re, im);
        }
        dst[idx] = fmaf(im, im, re * re);              // the square this launch has always fused
    }
}

// ---- complex STFT and its inverse (include/vc_hip.h, "Dereverberation"): the two halves of the filter kernels on their
// own, with the spectrum in global memory between them, planar and BIN-MAJOR: re, im [B][nb][maxF].  A tile of 16 frames
// goes through LDS as [bin][16], so every bin's run of the tile is 64 contiguous bytes on either side.
constexpr int ZT = 201 * VG;                           // elements of a 400-point tile, [bin][VG]
static_assert(ZT <= VG * 13 * VA_STRIDE, "the spectrum tile must fit the transform's rows");

__global__ void __launch_bounds__(VT)
stft_complex400_kernel(SfArgs a, float* __restrict__ re, float* __restrict__ im) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Tile400 t = carve400(smem);
    float *win = t.win, *Are = t.Are, *Aim = t.Aim, *xs = t.rest;      // Are / Aim: later the tile's spectrum [201][VG]

    const int b = blockIdx.y, tid = threadIdx.x;
    int len;
    const int F = sf_frames(a, b, len);
    const int f0 = blockIdx.x * VG;
    const int ncols = min(VG, a.maxF - f0);            // frames of the outputs this tile owns
    const size_t base = (size_t)b * 201 * a.maxF + f0;
    if (f0 >= F) {
        for (int i = tid; i < ZT; i += VT) {
            const int bin = i >> 4, g = i & 15;
            if (g < ncols) { re[base + (size_t)bin * a.maxF + g] = 0.0f; im[base + (size_t)bin * a.maxF + g] = 0.0f; }
        }
        return;
    }
    const int nvalid = min(VG, F - f0);

    copy_lds(win, a.window, 816);
    __syncthreads();
    sf_gather_tile(a, a.wav + (size_t)b * a.wav_stride, len, F, f0, xs);
    __syncthreads();
    // stft_power400_kernel's forward half: the two launches store and square the same re and im
    forward400_rows<vcfe::pinned::TW_POWER>(t, xs, a.hop, tid);
    __syncthreads();
    float yr[16], yi[16];
    if (tid < NROW) forward400_cols(t, tid, yr, yi);
    __syncthreads();                                   // every row of Are has been read
    if (tid < NROW) {
        const int g = tid / 13, k1 = tid - g * 13;
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            bool cj;
            const int bin = vcfe::src_bin(k1, k2, cj);
            // a slot above 200 holds the conjugate of its bin; each bin is stored by one slot (stft_power400_kernel)
            if (!cj || k1 != 0) {
                Are[bin * VG + g] = yr[k2];
                Aim[bin * VG + g] = cj ? -yi[k2] : yi[k2];
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < ZT; i += VT) {
        const int bin = i >> 4, g = i & 15;
        if (g < ncols) {
            re[base + (size_t)bin * a.maxF + g] = g < nvalid ? Are[i] : 0.0f;
            im[base + (size_t)bin * a.maxF + g] = g < nvalid ? Aim[i] : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(VT)
stft_complex_generic_kernel(SfArgs a, float* __restrict__ re, float* __restrict__ im) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, nb = a.nb;
    const TileGen t = carve_generic(smem, N);
    float *win = t.win, *twr = t.twr, *twi = t.twi, *xs = t.rest;    // [span]

    const int b = blockIdx.y, tid = threadIdx.x;
    int len;
    const int F = sf_frames(a, b, len);
    const int f0 = blockIdx.x * VGG;
    const int ncols = min(VGG, a.maxF - f0);
    const int nvalid = min(VGG, max(F - f0, 0));
    const size_t base = (size_t)b * nb * a.maxF + f0;
    if (nvalid > 0) {
        load_generic(t, a.window, N);
        __syncthreads();
        sf_gather_tile(a, a.wav + (size_t)b * a.wav_stride, len, F, f0, xs);
        __syncthreads();
    }
    for (int idx = tid; idx < VGG * nb; idx += VT) {
        const int k = idx / VGG, g = idx - k * VGG;
        if (g >= ncols) continue;
        float vr = 0.0f, vi = 0.0f;
        if (g < nvalid) forward_generic_bin(xs + g * a.hop, win, twr, twi, k, N, vr, vi);
        re[base + (size_t)k * a.maxF + g] = vr;
        im[base + (size_t)k * a.maxF + g] = vi;
    }
}

// The inverse half.  F_b = n_frames[b] clamped to [0, maxF] (null: maxF), 0 under the filter's "short" rule.
struct IzArgs {
    const float* re;         // [B][nb][maxF]
    const float* im;
    const int32_t* n_frames; // [B] or null
    float* frames;           // [B][maxF][N]
    int32_t* f_out;          // [B]: F_b for the overlap-add launch behind this one
    const float* window;     // [N] | tw400[416] | twg[2N]
    int maxF, nb, N, hop;
};

__device__ __forceinline__ int iz_frames(const IzArgs& a, int b) {
    int F = a.n_frames ? min(max(a.n_frames[b], 0), a.maxF) : a.maxF;
    if (a.hop * (F - 1) <= a.N / 2) F = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.f_out[b] = F;
    return F;
}

__global__ void __launch_bounds__(VT)
istft_complex400_kernel(IzArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Tile400 t = carve400(smem);
    float *win = t.win, *tw = t.tw, *Are = t.Are, *Aim = t.Aim;        // Are / Aim: first the tile's spectrum [201][VG]

    const int b = blockIdx.y, tid = threadIdx.x;
    const int F = iz_frames(a, b);
    const int f0 = blockIdx.x * VG;
    if (f0 >= F) return;
    const int nvalid = min(VG, F - f0);

    copy_lds(win, a.window, 816);
    const size_t base = (size_t)b * 201 * a.maxF + f0;
    for (int i = tid; i < ZT; i += VT) {
        const int bin = i >> 4, g = i & 15;
        const bool live = g < nvalid;
        Are[i] = live ? a.re[base + (size_t)bin * a.maxF + g] : 0.0f;
        // the imaginary parts of bin 0 and bin N / 2 are not read: a real frame has none
        Aim[i] = live && bin != 0 && bin != 200 ? a.im[base + (size_t)bin * a.maxF + g] : 0.0f;
    }
    __syncthreads();
    float zr[16], zi[16];
    const int gq = min(tid / 13, VG - 1), k1 = tid - (tid / 13) * 13;
    if (tid < NROW) {
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            bool cj;
            const int bin = vcfe::src_bin(k1, k2, cj);
            zr[k2] = Are[bin * VG + gq];
            zi[k2] = cj ? -Aim[bin * VG + gq] : Aim[bin * VG + gq];
        }
    }
    __syncthreads();                                   // the whole tile has been read
    if (tid < NROW) inverse400_cols(zr, zi, tw, Are, Aim, tid, k1);
    __syncthreads();
    inverse400_rows(Are, Aim, win, a.frames + ((size_t)b * a.maxF + f0) * 400, nvalid, tid);
}

__global__ void __launch_bounds__(VT)
istft_complex_generic_kernel(IzArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = a.N, nb = a.nb;
    const TileGen t = carve_generic(smem, N);
    float *win = t.win, *twr = t.twr, *twi = t.twi, *Sr = t.rest;    // [VGG][nb]
    float* Si = Sr + VGG * nb;

    const int b = blockIdx.y, tid = threadIdx.x;
    const int F = iz_frames(a, b);
    const int f0 = blockIdx.x * VGG;
    if (f0 >= F) return;
    const int nvalid = min(VGG, F - f0);
    load_generic(t, a.window, N);
    const size_t base = (size_t)b * nb * a.maxF + f0;
    for (int idx = tid; idx < VGG * nb; idx += VT) {
        const int k = idx / VGG, g = idx - k * VGG;
        const bool live = g < nvalid;
        Sr[g * nb + k] = live ? a.re[base + (size_t)k * a.maxF + g] : 0.0f;
        Si[g * nb + k] = live ? a.im[base + (size_t)k * a.maxF + g] : 0.0f;
    }
    __syncthreads();
    const float invN = 1.0f / (float)N;
    for (int idx = tid; idx < nvalid * N; idx += VT) {
        const int g = idx / N, n = idx - g * N;
        a.frames[((size_t)b * a.maxF + f0 + g) * N + n] =
            inverse_generic_sample(Sr + g * nb, Si + g * nb, win, twr, twi, n, N, nb, invN);
    }
}

// ---- the gain of the differential filter (include/vc_hip.h).  grid (tiles of gt frames, B).  A tile's differences go to
// LDS once, nb a frame; the smoothing reads them with the mirrored edges folded into the index (a bin whose taps all fall
// inside the row takes the plain loop).  Each lane then takes four consecutive elements of the tile's flat output.
constexpr int DG_MAX_TAPS = 65;

__device__ __forceinline__ int refl_bin(int i, int nb) {
    const int P = 2 * (nb - 1);
    int m = i % P;
    if (m < 0) m += P;
    return m < nb ? m : P - m;
}

// sum_j c[j] * d[.] ascending in j from +0, every product and every sum rounded on its own
__device__ __forceinline__ float smooth_rn(const float* c, const float* d, int k, int h, int nb) {
#pragma clang fp contract(off)
    float acc = 0.0f;
    if (k - h >= 0 && k + h < nb) {
        const float* p = d + (k - h);
        for (int j = 0; j <= 2 * h; ++j) { const float m = c[j] * p[j]; acc = acc + m; }
    } else {
        for (int j = 0; j <= 2 * h; ++j) { const float m = c[j] * d[refl_bin(k - h + j, nb)]; acc = acc + m; }
    }
    return acc;
}

template <bool VEC>
__global__ void __launch_bounds__(VT)
diff_gain_kernel(const float* __restrict__ pred, const float* __restrict__ tru, const int32_t* __restrict__ n_frames, int maxF,
                 int nb, int gt, float norm, float alpha, float boost, float cut, const float* __restrict__ taps, int n_taps,
                 float* __restrict__ gain) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* c = reinterpret_cast<float*>(smem);         // [DG_MAX_TAPS + 3]
    float* d = c + DG_MAX_TAPS + 3;                    // [gt][nb]
    const int b = blockIdx.y, tid = threadIdx.x;
    const int F = n_frames ? min(max(n_frames[b], 0), maxF) : maxF;
    const int f0 = blockIdx.x * gt;
    const int rows = min(gt, maxF - f0);               // rows of this tile inside the slab: all are written
    const int live = min(max(F - f0, 0), rows);        // ... of which these hold a gain
    const size_t base = ((size_t)b * maxF + f0) * nb;
    if (tid < n_taps) c[tid] = taps[tid];
    for (int i = tid; i < live * nb; i += VT)          // rows of 201 floats: element by element, as vc_compound_stitch reads
        d[i] = (fmaxf(pred[base + i], 0.0f) - fmaxf(tru[base + i], 0.0f)) / norm;
    __syncthreads();
    const int h = (n_taps - 1) / 2;
    const int total = rows * nb;
    for (int e0 = tid * 4; e0 < total; e0 += VT * 4) {
        float v[4];
        int g = e0 / nb, k = e0 - g * nb;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float G = 0.0f;
            if (g < live) {
                const float s0 = smooth_rn(c, d + g * nb, k, h, nb);
                const float s = fminf(fmaxf(alpha * s0, -cut), boost);
                G = exp2f(s * 0.16609640474436813f);   // float32(log2(10) / 20): power dB -> amplitude ratio
            }
            v[q] = G;
            if (++k == nb) { k = 0; ++g; }
        }
        if (VEC) {
            *reinterpret_cast<float4*>(gain + base + e0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e0 + q < total) gain[base + e0 + q] = v[q];
        }
    }
}

// wav[b][n] = trimmed, normalised overlap-add of the frames; optionally accumulates
// sum (wav - prev_wav)^2 into *delta (what the reference's verbose mode prints).
__global__ void __launch_bounds__(VT)
gl_ola_kernel(const float* frames, const int32_t* n_frames, const float* window, int maxF, int N, int hop, int nov,
              float* wav, int wav_stride, const float* prev_wav, int prev_stride, float* delta) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* win = reinterpret_cast<float*>(smem);
    const int b = blockIdx.y;
    const int F = n_frames ? min(max(n_frames[b], 0), maxF) : maxF;
    const int L = hop * (F - 1);
    copy_lds(win, window, N);
    __syncthreads();
    const int n = blockIdx.x * VT + threadIdx.x;
    float d2 = 0.0f;
    if (n < wav_stride) {
        float v = 0.0f;
        if (n < L) v = ola_at(frames + (size_t)b * maxF * N, win, n + N / 2, F, N, hop, nov);
        wav[(size_t)b * wav_stride + n] = v;
        if (delta && n < L) { const float d = v - prev_wav[(size_t)b * prev_stride + n]; d2 = d * d; }
    }
    if (delta) {
        d2 = vc::wave_sum(d2);
        if ((threadIdx.x & 63) == 0 && d2 != 0.0f) atomicAdd(delta + b, d2);
    }
}

// One block per utterance: y[n] = x[n] + c*y[n-1] (scipy.signal.lfilter([1],[1,-c])), then
// y *= target / mean|y|.  Each thread owns a contiguous chunk; chunk carries are combined with a
// scan over the affine maps  carry -> e_t + d_t * carry.
constexpr int PT = 1024;
__global__ void __launch_bounds__(PT)
inv_preemph_norm_kernel(float* wav, const int32_t* n_frames, int maxF, int hop, int stride, float coeff, float target) {
    __shared__ float sa[PT], sb[PT], red[PT / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int F = n_frames ? min(max(n_frames[b], 0), maxF) : maxF;
    const int L = min(hop * (F - 1), stride);
    float* y = wav + (size_t)b * stride;
    const int C = (L + PT - 1) / PT;
    const int s0 = min(t * C, L), s1 = min(s0 + C, L);
    float asum = 0.0f;
    if (coeff != 0.0f) {
        float carry = 0.0f, d = 1.0f;
        for (int n = s0; n < s1; ++n) { carry = fmaf(coeff, carry, y[n]); y[n] = carry; d *= coeff; }
        sa[t] = d; sb[t] = carry;
        __syncthreads();
        for (int off = 1; off < PT; off <<= 1) {          // inclusive scan of (a, b): later o earlier
            float a1 = 1.0f, b1 = 0.0f;
            if (t >= off) { a1 = sa[t - off]; b1 = sb[t - off]; }
            __syncthreads();
            if (t >= off) { sb[t] = fmaf(sa[t], b1, sb[t]); sa[t] *= a1; }
            __syncthreads();
        }
        const float cin = t > 0 ? sb[t - 1] : 0.0f;
        float pw = coeff;
        for (int n = s0; n < s1; ++n) { const float v = fmaf(pw, cin, y[n]); y[n] = v; asum += fabsf(v); pw *= coeff; }
    } else {
        for (int n = s0; n < s1; ++n) asum += fabsf(y[n]);
    }
    asum = vc::wave_sum(asum);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = asum;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int i = 0; i < PT / 64; ++i) tot += red[i];
    const float sc = (L > 0 && tot > 0.0f) ? target / (tot / (float)L) : 1.0f;
    if (target > 0.0f)
        for (int n = s0; n < s1; ++n) y[n] *= sc;
}

// One block per utterance: audio_lib.py:289-298.  P [F][nb] -> amplitude [F][nb].
__global__ void __launch_bounds__(PT)
power_to_amp_kernel(const float* P, const int32_t* n_frames, int maxF, int nb, float inv_norm, float realse, float* amp) {
    __shared__ float r0[PT / 64], r1[PT / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int F = n_frames ? min(max(n_frames[b], 0), maxF) : maxF;
    const size_t total = (size_t)F * nb, all = (size_t)maxF * nb;
    const float* p = P + (size_t)b * all;
    float* o = amp + (size_t)b * all;
    float gain = 1.0f;
    if (realse != 1.0f) {
        float s0 = 0.0f, s1 = 0.0f;
        for (size_t i = t; i < total; i += PT) {
            const float v = fmaxf(0.0f, p[i]);
            s0 += v; s1 += powf(v, realse);
        }
        s0 = vc::wave_sum(s0); s1 = vc::wave_sum(s1);
        if ((t & 63) == 0) { r0[t >> 6] = s0; r1[t >> 6] = s1; }
        __syncthreads();
        float t0 = 0.0f, t1 = 0.0f;
#pragma unroll
        for (int i = 0; i < PT / 64; ++i) { t0 += r0[i]; t1 += r1[i]; }
        gain = t0 / t1;                                  // p_mean / mean(P ** realse)
    }
    for (size_t i = t; i < all; i += PT) {
        float v = 0.0f;
        if (i < total) {
            v = fmaxf(0.0f, p[i]);
            if (realse != 1.0f) v = gain * powf(v, realse);
            v = exp10f(0.05f * (v * inv_norm - 80.0f));  // sqrt(db_to_power(P/norm - 80))
        }
        o[i] = v;
    }
}

}  // namespace

struct vc_vocoder_plan {
    int32_t win_length, hop, N, nb, nov, span, span_g;
    float* d_tables;       // window[N] | tw400[416] | twg[2N]
    size_t smem400, smem400_init, smem_gen;
};

// Bytes of the ping-pong frames and (trace) the two scratch waveforms, each rounded to 256.
static size_t gl_state_offset(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames, int32_t trace) {
    size_t frames = (size_t)batch * max_frames * plan->N * sizeof(float);
    frames = (frames + 255) & ~(size_t)255;
    size_t wav = trace ? (((size_t)batch * plan->hop * (max_frames - 1) * sizeof(float) + 255) & ~(size_t)255) : 0;
    return 2 * frames + 2 * wav;
}

// Momentum state: one float2 per slot the iteration kernel projects (400: 13 x 16, generic: nb).
static size_t gl_mom_bytes(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames) {
    const size_t slots = plan->N == 400 ? (size_t)NSLOT400 : (size_t)plan->nb;
    return ((size_t)batch * max_frames * slots * sizeof(float2) + 255) & ~(size_t)255;
}

// Both entry points: momentum == 0 launches exactly the plain instantiations (MOM_OFF).
static int griffin_lim_run(const char* fn, const vc_vocoder_plan* p, const float* d_amp, const float* d_phase0,
                           const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t num_iters,
                           float momentum, float* d_wav, int32_t wav_stride, float* d_trace, void* d_workspace,
                           size_t workspace_bytes, void* stream) {
    VC_REQUIRE(p && d_amp && d_phase0 && d_wav && d_workspace, "%s: NULL argument", fn);
    VC_REQUIRE(batch > 0 && max_frames >= 2 && num_iters >= 1, "%s: need batch > 0, frames >= 2, num_iters >= 1", fn);
    VC_REQUIRE(std::isfinite(momentum) && momentum >= 0.0f && momentum < 1.0f,
               "%s: momentum must be finite and in [0, 1) (got %g)", fn, (double)momentum);
    VC_REQUIRE(p->hop * (max_frames - 1) > p->N / 2, "%s: %d frames are shorter than the reflect padding", fn, max_frames);
    VC_REQUIRE(wav_stride >= p->hop * (max_frames - 1), "%s: wav_stride %d < %d samples", fn, wav_stride,
               p->hop * (max_frames - 1));
    const bool mom = momentum > 0.0f;
    const int32_t tr = d_trace != nullptr;
    const size_t need = mom ? vc_vocoder_workspace_bytes_momentum(p, batch, max_frames, tr)
                            : vc_vocoder_workspace_bytes(p, batch, max_frames, tr);
    VC_REQUIRE(workspace_bytes >= need, "%s: workspace too small", fn);
    VC_REQUIRE(!mom || ((uintptr_t)d_workspace & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    size_t fbytes = ((size_t)batch * max_frames * p->N * sizeof(float) + 255) & ~(size_t)255;
    float* fr[2] = {reinterpret_cast<float*>(d_workspace), reinterpret_cast<float*>((char*)d_workspace + fbytes)};
    const int L = p->hop * (max_frames - 1);
    const size_t wbytes = ((size_t)batch * L * sizeof(float) + 255) & ~(size_t)255;
    float* wavs[2] = {reinterpret_cast<float*>((char*)d_workspace + 2 * fbytes),
                      reinterpret_cast<float*>((char*)d_workspace + 2 * fbytes + wbytes)};
    const bool fast = (p->N == 400);
    GlArgs a;
    a.amp = d_amp; a.phase0 = d_phase0; a.n_frames = d_n_frames; a.window = p->d_tables;
    a.maxF = max_frames; a.nb = p->nb; a.N = p->N; a.hop = p->hop; a.nov = p->nov;
    a.span = fast ? p->span : p->span_g;
    a.mom = mom ? reinterpret_cast<float2*>((char*)d_workspace + gl_state_offset(p, batch, max_frames, tr))
                : nullptr;
    a.beta = (float)((double)momentum / (1.0 + (double)momentum));
    const dim3 grid(((unsigned)max_frames + (fast ? VG : VGG) - 1) / (fast ? VG : VGG), (unsigned)batch);
    const size_t smem = fast ? p->smem400 : p->smem_gen;
    if (int rc = vc::allow_dynamic_lds<gl_iter_generic_kernel<true, MOM_OFF>,
                                       gl_iter_generic_kernel<false, MOM_OFF>,
                                       gl_iter_generic_kernel<false, MOM_FIRST>,
                                       gl_iter_generic_kernel<false, MOM_ON>,
                                       gl_iter400_kernel<true, MOM_OFF>,
                                       gl_iter400_kernel<false, MOM_OFF>,
                                       gl_iter400_kernel<false, MOM_FIRST>,
                                       gl_iter400_kernel<false, MOM_ON>>(160 * 1024)) return rc;
    const dim3 ogrid(((unsigned)wav_stride + VT - 1) / VT, (unsigned)batch);
    const dim3 sgrid(((unsigned)L + VT - 1) / VT, (unsigned)batch);
    const size_t osmem = (size_t)p->N * sizeof(float);
    const bool trace = d_trace != nullptr;
    if (trace) VC_HIP_CHECK(vc::zero_async(d_trace, sizeof(float) * (size_t)num_iters * batch, st));
    // iteration i leaves the frames of waveform i in fr[cur]; trace mode also materialises every
    // intermediate waveform (scratch, stride L) to accumulate sum (wav_i - wav_{i-1})^2.
    int cur = 0;
    for (int i = 0; i < num_iters; ++i) {
        a.prev = fr[cur]; a.next = fr[cur ^ 1];
        if (i == 0) {
            if (fast) hipLaunchKernelGGL((gl_iter400_kernel<true, MOM_OFF>), grid, dim3(VT), p->smem400_init, st, a);
            else hipLaunchKernelGGL((gl_iter_generic_kernel<true, MOM_OFF>), grid, dim3(VT), smem, st, a);
        } else if (!mom) {
            if (fast) hipLaunchKernelGGL((gl_iter400_kernel<false, MOM_OFF>), grid, dim3(VT), smem, st, a);
            else hipLaunchKernelGGL((gl_iter_generic_kernel<false, MOM_OFF>), grid, dim3(VT), smem, st, a);
        } else if (i == 1) {                           // R_0 = 0: the state is written, not read
            if (fast) hipLaunchKernelGGL((gl_iter400_kernel<false, MOM_FIRST>), grid, dim3(VT), smem, st, a);
            else hipLaunchKernelGGL((gl_iter_generic_kernel<false, MOM_FIRST>), grid, dim3(VT), smem, st, a);
        } else {
            if (fast) hipLaunchKernelGGL((gl_iter400_kernel<false, MOM_ON>), grid, dim3(VT), smem, st, a);
            else hipLaunchKernelGGL((gl_iter_generic_kernel<false, MOM_ON>), grid, dim3(VT), smem, st, a);
        }
        cur ^= 1;
        if (trace && i < num_iters - 1)
            hipLaunchKernelGGL(gl_ola_kernel, sgrid, dim3(VT), osmem, st, fr[cur], d_n_frames, p->d_tables, max_frames,
                               p->N, p->hop, p->nov, wavs[i & 1], L, (const float*)(i > 0 ? wavs[(i - 1) & 1] : nullptr), L,
                               i > 0 ? d_trace + (size_t)i * batch : (float*)nullptr);
    }
    const bool last_delta = trace && num_iters > 1;
    hipLaunchKernelGGL(gl_ola_kernel, ogrid, dim3(VT), osmem, st, fr[cur], d_n_frames, p->d_tables, max_frames, p->N,
                       p->hop, p->nov, d_wav, wav_stride, (const float*)(last_delta ? wavs[(num_iters - 2) & 1] : nullptr), L,
                       last_delta ? d_trace + (size_t)(num_iters - 1) * batch : (float*)nullptr);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

extern "C" {

int vc_vocoder_plan_create(int32_t win_length, int32_t hop_length, int32_t n_fft, const double* h_window,
                           vc_vocoder_plan** out_plan) {
    VC_REQUIRE(out_plan, "out_plan is NULL");
    if (n_fft <= 0) n_fft = win_length;
    VC_REQUIRE(win_length > 0 && hop_length > 0 && n_fft >= win_length && (n_fft % 2) == 0 && n_fft <= 4096,
               "vocoder: need 0 < win_length <= n_fft <= 4096, n_fft even, hop_length > 0 (got %d, %d, %d)",
               win_length, n_fft, hop_length);
    VC_REQUIRE(hop_length <= n_fft, "vocoder: hop_length %d > n_fft %d leaves gaps", hop_length, n_fft);
    const double PI = 3.14159265358979323846;
    const int N = n_fft;
    std::vector<float> h((size_t)3 * N + 416, 0.0f);
    const int lpad = (N - win_length) / 2;
    for (int i = 0; i < win_length; ++i)
        h[lpad + i] = (float)(h_window ? h_window[i] : 0.5 - 0.5 * std::cos(2.0 * PI * i / win_length));
    for (int k1 = 0; k1 < 13; ++k1)
        for (int n2 = 0; n2 < 16; ++n2) {
            const double ang = -2.0 * PI * (double)(n2 * k1) / 400.0;
            h[N + k1 * 16 + n2] = (float)std::cos(ang);
            h[N + 208 + k1 * 16 + n2] = (float)std::sin(ang);
        }
    for (int m = 0; m < N; ++m) {
        const double ang = -2.0 * PI * (double)m / (double)N;
        h[N + 416 + m] = (float)std::cos(ang);
        h[N + 416 + N + m] = (float)std::sin(ang);
    }
    vc_vocoder_plan* p = new vc_vocoder_plan();
    p->win_length = win_length; p->hop = hop_length; p->N = N; p->nb = 1 + N / 2;
    p->nov = (N + hop_length - 1) / hop_length;
    p->span = (VG - 1) * hop_length + N;
    p->span_g = (VGG - 1) * hop_length + N;
    p->d_tables = nullptr;
    if (hipMalloc(&p->d_tables, h.size() * 4) != hipSuccess) {
        delete p;
        return vc::set_error(VC_ERR_HIP, "vocoder plan: hipMalloc failed");
    }
    if (hipMemcpy(p->d_tables, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p->d_tables); delete p;
        return vc::set_error(VC_ERR_HIP, "vocoder plan: hipMemcpy failed");
    }
    p->smem400 = sizeof(float) * (400 + 416 + 2 * (VG * 13) * VA_STRIDE + (size_t)p->span);
    p->smem400_init = sizeof(float) * (400 + 416 + 2 * (VG * 13) * VA_STRIDE + 2 * VG * 201);
    p->smem_gen = sizeof(float) * ((size_t)3 * N + 2 * VGG * p->nb + p->span_g);
    if (N != 400 && p->smem_gen > 160 * 1024) {
        (void)hipFree(p->d_tables); delete p;
        return vc::set_error(VC_ERR_INVALID, "vocoder: n_fft %d needs %zu bytes of LDS", N, p->smem_gen);
    }
    *out_plan = p;
    return VC_OK;
}

void vc_vocoder_plan_destroy(vc_vocoder_plan* plan) {
    if (!plan) return;
    if (plan->d_tables) (void)hipFree(plan->d_tables);
    delete plan;
}

int32_t vc_vocoder_num_samples(const vc_vocoder_plan* plan, int32_t n_frames) {
    return plan && n_frames > 0 ? plan->hop * (n_frames - 1) : 0;
}

size_t vc_vocoder_workspace_bytes(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames, int32_t trace) {
    if (!plan || batch <= 0 || max_frames <= 0) return 0;
    return gl_state_offset(plan, batch, max_frames, trace) + 256;
}

size_t vc_vocoder_workspace_bytes_momentum(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames,
                                           int32_t trace) {
    if (!plan || batch <= 0 || max_frames <= 0) return 0;
    return gl_state_offset(plan, batch, max_frames, trace) + gl_mom_bytes(plan, batch, max_frames) + 256;
}

int vc_power_to_amp(const float* d_P, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_bins,
                    float P_dB_norm_factor, float realse, float* d_amp, void* stream) {
    VC_REQUIRE(d_P && d_amp && batch > 0 && max_frames > 0 && n_bins > 0, "vc_power_to_amp: bad arguments");
    VC_REQUIRE(P_dB_norm_factor != 0.0f, "vc_power_to_amp: P_dB_norm_factor is 0");
    hipLaunchKernelGGL(power_to_amp_kernel, dim3(batch), dim3(PT), 0, (hipStream_t)stream, d_P, d_n_frames, max_frames,
                       n_bins, 1.0f / P_dB_norm_factor, realse, d_amp);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_griffin_lim_f32(const vc_vocoder_plan* p, const float* d_amp, const float* d_phase0, const int32_t* d_n_frames,
                       int32_t batch, int32_t max_frames, int32_t num_iters, float* d_wav, int32_t wav_stride,
                       float* d_trace, void* d_workspace, size_t workspace_bytes, void* stream) {
    return griffin_lim_run("vc_griffin_lim_f32", p, d_amp, d_phase0, d_n_frames, batch, max_frames, num_iters, 0.0f,
                           d_wav, wav_stride, d_trace, d_workspace, workspace_bytes, stream);
}

int vc_griffin_lim_momentum_f32(const vc_vocoder_plan* p, const float* d_amp, const float* d_phase0,
                                const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t num_iters,
                                float momentum, float* d_wav, int32_t wav_stride, float* d_trace, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    return griffin_lim_run("vc_griffin_lim_momentum_f32", p, d_amp, d_phase0, d_n_frames, batch, max_frames, num_iters,
                           momentum, d_wav, wav_stride, d_trace, d_workspace, workspace_bytes, stream);
}

int vc_inv_preemphasis_normalize(const vc_vocoder_plan* p, float* d_wav, const int32_t* d_n_frames, int32_t batch,
                                 int32_t max_frames, int32_t wav_stride, float coeff, float mean_abs_amp_norm, void* stream) {
    VC_REQUIRE(p && d_wav && batch > 0 && max_frames >= 1 && wav_stride >= 0, "vc_inv_preemphasis_normalize: bad arguments");
    hipLaunchKernelGGL(inv_preemph_norm_kernel, dim3(batch), dim3(PT), 0, (hipStream_t)stream, d_wav, d_n_frames, max_frames,
                       p->hop, wav_stride, coeff, mean_abs_amp_norm);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_spectral_diff_gain_f32(const float* d_pred, const float* d_true, const int32_t* d_n_frames, int32_t batch,
                              int32_t max_frames, int32_t n_bins, float P_dB_norm_factor, float alpha, float max_boost_db,
                              float max_cut_db, const float* d_taps, int32_t n_taps, float* d_gain, void* stream) {
    const char* fn = "vc_spectral_diff_gain_f32";
    VC_REQUIRE(d_pred && d_true && d_taps && d_gain, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && n_bins >= 2 && n_bins <= 2049,
               "%s: bad shape (batch %d in [1, 65535], max_frames %d >= 1, n_bins %d in [2, 2049])", fn, batch, max_frames, n_bins);
    VC_REQUIRE(n_taps >= 1 && n_taps <= DG_MAX_TAPS && (n_taps & 1), "%s: n_taps must be odd and in [1, %d] (got %d)", fn,
               DG_MAX_TAPS, n_taps);
    VC_REQUIRE(std::isfinite(P_dB_norm_factor) && P_dB_norm_factor != 0.0f && std::isfinite(alpha) &&
               std::isfinite(max_boost_db) && std::isfinite(max_cut_db), "%s: a float argument is not finite, or P_dB_norm_factor is 0", fn);
    VC_REQUIRE(alpha >= 0.0f && alpha <= 1.0f, "%s: alpha must be in [0, 1] (got %g)", fn, (double)alpha);
    VC_REQUIRE(max_boost_db >= 0.0f && max_cut_db >= 0.0f, "%s: the clamps must not be negative (got %g, %g)", fn,
               (double)max_boost_db, (double)max_cut_db);
    VC_REQUIRE((long long)max_frames * n_bins < (1ll << 31), "%s: an utterance holds more than 2^31 values", fn);
    // 16 frames a tile while their differences fit 64 KB of LDS with the taps, else 4 (n_bins <= 2049: 33 KB)
    const int gt = (size_t)16 * n_bins * sizeof(float) <= 60 * 1024 ? 16 : 4;
    const size_t smem = sizeof(float) * ((size_t)DG_MAX_TAPS + 3 + (size_t)gt * n_bins);
    const dim3 grid(((unsigned)max_frames + gt - 1) / gt, (unsigned)batch);
    const bool vec = ((long long)max_frames * n_bins) % 4 == 0 && ((uintptr_t)d_gain & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL((diff_gain_kernel<true>), grid, dim3(VT), smem, st, d_pred, d_true, d_n_frames, max_frames, n_bins, gt,
                           P_dB_norm_factor, alpha, max_boost_db, max_cut_db, d_taps, n_taps, d_gain);
    else
        hipLaunchKernelGGL((diff_gain_kernel<false>), grid, dim3(VT), smem, st, d_pred, d_true, d_n_frames, max_frames, n_bins, gt,
                           P_dB_norm_factor, alpha, max_boost_db, max_cut_db, d_taps, n_taps, d_gain);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

// frame buffer, then the table F_b [batch] int32 the filter kernel leaves for the overlap-add (the spare bytes up to 64
// utterances, rounded up to 256 beyond)
static size_t sf_frames_bytes(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames) {
    return ((size_t)batch * max_frames * plan->N * sizeof(float) + 255) & ~(size_t)255;
}

size_t vc_stft_filter_workspace_bytes(const vc_vocoder_plan* plan, int32_t batch, int32_t max_frames) {
    if (!plan || batch <= 0 || max_frames <= 0) return 0;
    return sf_frames_bytes(plan, batch, max_frames) + (((size_t)batch * sizeof(int32_t) + 255) & ~(size_t)255);
}

int vc_stft_filter_f32(const vc_vocoder_plan* p, const float* d_wav, int32_t wav_stride, const int32_t* d_len,
                       const float* d_gain, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float* d_out,
                       int32_t out_stride, void* d_workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "vc_stft_filter_f32";
    VC_REQUIRE(p && d_wav && d_len && d_gain && d_out && d_workspace, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && wav_stride >= 1,
               "%s: bad shape (batch %d in [1, 65535], max_frames %d >= 1, wav_stride %d >= 1)", fn, batch, max_frames, wav_stride);
    VC_REQUIRE((long long)p->hop * (max_frames - 1) + p->N < (1ll << 31), "%s: %d frames exceed 2^31 samples", fn, max_frames);
    VC_REQUIRE(out_stride >= p->hop * (max_frames - 1) && out_stride >= 1, "%s: out_stride %d < %d samples", fn, out_stride,
               p->hop * (max_frames - 1));
    VC_REQUIRE(((uintptr_t)d_workspace & 3) == 0, "%s: workspace must be 4-byte aligned", fn);
    if (workspace_bytes < vc_stft_filter_workspace_bytes(p, batch, max_frames))
        return vc::set_error(VC_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes,
                             vc_stft_filter_workspace_bytes(p, batch, max_frames));
    const bool fast = (p->N == 400);
    if (int rc = vc::allow_dynamic_lds<stft_filter400_kernel, stft_filter_generic_kernel>(160 * 1024)) return rc;
    SfArgs a;
    a.wav = d_wav; a.len = d_len; a.gain = d_gain; a.n_frames = d_n_frames;
    a.frames = reinterpret_cast<float*>(d_workspace);
    a.f_out = reinterpret_cast<int32_t*>((char*)d_workspace + sf_frames_bytes(p, batch, max_frames));
    a.window = p->d_tables;
    a.wav_stride = wav_stride; a.maxF = max_frames; a.nb = p->nb; a.N = p->N; a.hop = p->hop;
    a.span = fast ? p->span : p->span_g;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(((unsigned)max_frames + (fast ? VG : VGG) - 1) / (fast ? VG : VGG), (unsigned)batch);
    if (fast) hipLaunchKernelGGL(stft_filter400_kernel, grid, dim3(VT), p->smem400, st, a);
    else hipLaunchKernelGGL(stft_filter_generic_kernel, grid, dim3(VT), p->smem_gen, st, a);
    const dim3 ogrid(((unsigned)out_stride + VT - 1) / VT, (unsigned)batch);
    hipLaunchKernelGGL(gl_ola_kernel, ogrid, dim3(VT), (size_t)p->N * sizeof(float), st, a.frames, a.f_out, p->d_tables,
                       max_frames, p->N, p->hop, p->nov, d_out, out_stride, (const float*)nullptr, 0, (float*)nullptr);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_stft_power_f32(const vc_vocoder_plan* p, const float* d_wav, int32_t wav_stride, const int32_t* d_len,
                      const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float* d_power, int32_t* d_frames_out,
                      void* stream) {
    const char* fn = "vc_stft_power_f32";
    VC_REQUIRE(p && d_wav && d_len && d_power && d_frames_out, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && wav_stride >= 1,
               "%s: bad shape (batch %d in [1, 65535], max_frames %d >= 1, wav_stride %d >= 1)", fn, batch, max_frames, wav_stride);
    VC_REQUIRE((long long)p->hop * (max_frames - 1) + p->N < (1ll << 31), "%s: %d frames exceed 2^31 samples", fn, max_frames);
    const bool fast = (p->N == 400);
    if (int rc = vc::allow_dynamic_lds<stft_power400_kernel, stft_power_generic_kernel>(160 * 1024)) return rc;
    SfArgs a;
    a.wav = d_wav; a.len = d_len; a.gain = nullptr; a.n_frames = d_n_frames; a.frames = nullptr; a.f_out = d_frames_out;
    a.window = p->d_tables;
    a.wav_stride = wav_stride; a.maxF = max_frames; a.nb = p->nb; a.N = p->N; a.hop = p->hop;
    a.span = fast ? p->span : p->span_g;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(((unsigned)max_frames + (fast ? VG : VGG) - 1) / (fast ? VG : VGG), (unsigned)batch);
    if (fast) hipLaunchKernelGGL(stft_power400_kernel, grid, dim3(VT), p->smem400, st, a, d_power);
    else hipLaunchKernelGGL(stft_power_generic_kernel, grid, dim3(VT), p->smem_gen, st, a, d_power);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_stft_complex_f32(const vc_vocoder_plan* p, const float* d_wav, int32_t wav_stride, const int32_t* d_len,
                        const int32_t* d_n_frames, int32_t batch, int32_t max_frames, float* d_re, float* d_im,
                        int32_t* d_frames_out, void* stream) {
    const char* fn = "vc_stft_complex_f32";
    VC_REQUIRE(p && d_wav && d_len && d_re && d_im && d_frames_out, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1 && wav_stride >= 1,
               "%s: bad shape (batch %d in [1, 65535], max_frames %d >= 1, wav_stride %d >= 1)", fn, batch, max_frames, wav_stride);
    VC_REQUIRE((long long)p->hop * (max_frames - 1) + p->N < (1ll << 31), "%s: %d frames exceed 2^31 samples", fn, max_frames);
    const bool fast = (p->N == 400);
    if (int rc = vc::allow_dynamic_lds<stft_complex400_kernel, stft_complex_generic_kernel>(160 * 1024)) return rc;
    SfArgs a;
    a.wav = d_wav; a.len = d_len; a.gain = nullptr; a.n_frames = d_n_frames; a.frames = nullptr; a.f_out = d_frames_out;
    a.window = p->d_tables;
    a.wav_stride = wav_stride; a.maxF = max_frames; a.nb = p->nb; a.N = p->N; a.hop = p->hop;
    a.span = fast ? p->span : p->span_g;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(((unsigned)max_frames + (fast ? VG : VGG) - 1) / (fast ? VG : VGG), (unsigned)batch);
    if (fast) hipLaunchKernelGGL(stft_complex400_kernel, grid, dim3(VT), p->smem400, st, a, d_re, d_im);
    else hipLaunchKernelGGL(stft_complex_generic_kernel, grid, dim3(VT), p->smem_gen, st, a, d_re, d_im);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_istft_complex_f32(const vc_vocoder_plan* p, const float* d_re, const float* d_im, const int32_t* d_n_frames,
                         int32_t batch, int32_t max_frames, float* d_out, int32_t out_stride, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
    const char* fn = "vc_istft_complex_f32";
    VC_REQUIRE(p && d_re && d_im && d_out && d_workspace, "%s: NULL argument", fn);
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_frames >= 1, "%s: bad shape (batch %d in [1, 65535], max_frames %d >= 1)", fn,
               batch, max_frames);
    VC_REQUIRE((long long)p->hop * (max_frames - 1) + p->N < (1ll << 31), "%s: %d frames exceed 2^31 samples", fn, max_frames);
    VC_REQUIRE(out_stride >= p->hop * (max_frames - 1) && out_stride >= 1, "%s: out_stride %d < %d samples", fn, out_stride,
               p->hop * (max_frames - 1));
    VC_REQUIRE(((uintptr_t)d_workspace & 3) == 0, "%s: workspace must be 4-byte aligned", fn);
    if (workspace_bytes < vc_stft_filter_workspace_bytes(p, batch, max_frames))
        return vc::set_error(VC_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes,
                             vc_stft_filter_workspace_bytes(p, batch, max_frames));
    const bool fast = (p->N == 400);
    if (int rc = vc::allow_dynamic_lds<istft_complex400_kernel, istft_complex_generic_kernel>(160 * 1024)) return rc;
    IzArgs a;
    a.re = d_re; a.im = d_im; a.n_frames = d_n_frames;
    a.frames = reinterpret_cast<float*>(d_workspace);
    a.f_out = reinterpret_cast<int32_t*>((char*)d_workspace + sf_frames_bytes(p, batch, max_frames));
    a.window = p->d_tables;
    a.maxF = max_frames; a.nb = p->nb; a.N = p->N; a.hop = p->hop;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(((unsigned)max_frames + (fast ? VG : VGG) - 1) / (fast ? VG : VGG), (unsigned)batch);
    if (fast) hipLaunchKernelGGL(istft_complex400_kernel, grid, dim3(VT), p->smem400, st, a);
    else hipLaunchKernelGGL(istft_complex_generic_kernel, grid, dim3(VT), p->smem_gen, st, a);
    const dim3 ogrid(((unsigned)out_stride + VT - 1) / VT, (unsigned)batch);
    hipLaunchKernelGGL(gl_ola_kernel, ogrid, dim3(VT), (size_t)p->N * sizeof(float), st, a.frames, a.f_out, p->d_tables,
                       max_frames, p->N, p->hop, p->nov, d_out, out_stride, (const float*)nullptr, 0, (float*)nullptr);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
