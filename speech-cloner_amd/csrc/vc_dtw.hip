// Scoring conversions on the device (include/vc_hip.h, "Evaluation"): mel cepstra, dynamic time warping over the
// mel-cepstral frame distance, the back-track of its path, and the frame-synchronous mean.
//
//     c[f, d]  = sum_m Dct[d, m] * mel[f, m]                                          (vc_mel_cepstra)
//     d(i, j)  = scale * sqrt(2 * sum_d (ca[i, d] - cb[j, d])^2)
//     D(i, j)  = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)),  D(0, 0) = d(0, 0)  (vc_dtw_f32)
//     L(i, j)  = 1 + L(predecessor), L(0, 0) = 1;   ties take the predecessor in the order diagonal, up, left
//
// No Fa x Fb matrix of costs or distances exists anywhere: d(i, j) is computed in the lane that consumes it, from the
// lane's own rows of A (registers) and a window of B's cepstra (LDS).
//
// One workgroup per pair, NT = 256 lanes, R = 4 consecutive rows of A per lane: a pass covers NT * R = 1,024 rows.  Lane t
// works on column j = s - t at step s, so the lanes of a pass form one anti-diagonal of the lane grid, and what lane t
// needs from above -- D and L of lane t-1's last row at columns j and j-1 -- was produced at steps s-1 and s-2.  Every
// lane stores the (D, L) of its last row in LDS after its step (two buffers by step parity), one barrier ends the step, and
// the next step's first instruction reads the neighbour's pair; the value read one step earlier is the diagonal.  The read
// is issued before the 2 * R * n_coef vector operations of the distances and is consumed after them.  Lane 0 reads the
// boundary row left by the previous pass instead (+inf in the first pass), staged in LDS with B's cepstra.
//
// B's cepstra live in a ring of 2 * NT columns, row stride NC + 4 floats: lanes read consecutive columns with 16-byte
// reads, and 16 consecutive rows of that stride fall on the 64 banks exactly once (28 j mod 64 and 36 j mod 64 run through
// every multiple of 4; strides 12 and 20 likewise -- by this arithmetic, not measured with counters).  Every NT steps
// the half of the ring that no lane can still need is refilled: the columns in flight at steps [c NT, (c+1) NT) lie in
// chunks c-1 and c.
//
// Rows beyond 1,024 take further passes; the last row of a pass goes through two rows of (D, L) per pair in the
// workspace (written by the pass's last lane, read back by the whole workgroup chunk by chunk after a barrier).  That is
// the O(Fb) workspace of score mode.  Path mode adds two bits per cell (0 diagonal, 1 up, 2 left), sixteen columns to
// a word, collected in registers and stored once per sixteen steps; vc_dtw_backtrack walks them from the end cell.
//
// A pair's result depends on that pair alone and on nothing that varies from run to run: fixed lane geometry, one
// summation order per distance (d = 0 .. n_coef-1, fused multiply-adds), no atomics.
#include <cmath>
#include <mutex>
#include "vc_device.h"

namespace {

constexpr int NT = 256;                 // lanes per workgroup (four waves, one per SIMD)
constexpr int R = 4;                    // rows of A per lane
constexpr int ROWS = NT * R;            // rows per pass
constexpr int RING = 2 * NT;            // columns of B kept in LDS
constexpr int MAX_FRAMES = 16384;       // 2^14: j * (Fa - 1) stays below 2^28
constexpr int MAX_COEF = 32;
constexpr long long MAX_CODE_BYTES = 1ll << 31;      // path mode: packed predecessor codes of the whole batch

struct Cell {                           // accumulated cost and path length of one cell
    float D;
    int32_t L;
};

inline size_t boundary_bytes(int batch, int max_b) { return vc::align256((size_t)batch * 2 * max_b * sizeof(Cell)); }
inline int words_per_row(int max_b) { return (max_b + 15) >> 4; }

template <int NC>
constexpr int dtw_lds_bytes() {
    return RING * (NC + 4) * 4 + RING * (int)sizeof(Cell) + 2 * NT * (int)sizeof(Cell);
}

// cepstra of A: ca [batch, max_a, n_coef]; of B: cb [batch, max_b, n_coef].  bound [batch][2][max_b] Cells.
// codes [batch][max_a][wpr] words or NULL.  limit < 0: no band.
template <int NC, bool PATH>
__global__ void __launch_bounds__(NT)
dtw_kernel(const float* __restrict__ ca, const float* __restrict__ cb, const int32_t* __restrict__ len_a,
           const int32_t* __restrict__ len_b, int max_a, int max_b, int n_coef, float scale, int band,
           float* __restrict__ total, int32_t* __restrict__ path_len, float* __restrict__ mcd, Cell* __restrict__ bound,
           uint32_t* __restrict__ codes, int wpr) {
    constexpr int STR = NC + 4;
    extern __shared__ __align__(16) float lds[];
    float* ring = lds;                                              // [RING][STR]
    Cell* top = reinterpret_cast<Cell*>(lds + RING * STR);          // [RING]: the row above the pass, by column
    Cell* hand = top + RING;                                        // [2][NT]: every lane's last row, by step parity
    const int p = blockIdx.x;
    const int t = threadIdx.x;
    const int Fa = min(max(len_a[p], 1), max_a);
    const int Fb = min(max(len_b[p], 1), max_b);
    const float* __restrict__ A = ca + (size_t)p * max_a * n_coef;
    const float* __restrict__ B = cb + (size_t)p * max_b * n_coef;
    Cell* bnd = bound + (size_t)p * 2 * max_b;
    uint32_t* cw = PATH ? codes + (size_t)p * max_a * wpr : nullptr;
    const float INF = __builtin_inff();
    const long long limit = band < 0 ? -1 : (long long)band * max(Fa - 1, Fb - 1);
    const int fa1 = Fa - 1, fb1 = Fb - 1;

    for (int i = t; i < RING * STR; i += NT) ring[i] = 0.0f;       // the padding d >= n_coef stays zero for good
    const int n_pass = (Fa + ROWS - 1) / ROWS;
    for (int ps = 0; ps < n_pass; ++ps) {
        const int i0 = ps * ROWS + t * R;                           // this lane's first row
        const int rows_here = min(ROWS, Fa - ps * ROWS);
        const int t_last = (rows_here - 1) / R;
        const bool last_pass = ps == n_pass - 1;
        const Cell* bin = bnd + (size_t)(ps & 1) * max_b;           // written by pass ps - 1
        Cell* bout = bnd + (size_t)((ps + 1) & 1) * max_b;
        float a[R][NC];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int d = 0; d < NC; ++d) a[r][d] = (i0 + r < Fa && d < n_coef) ? A[(size_t)(i0 + r) * n_coef + d] : 0.0f;
        float Dl[R];                                                // column j - 1 of this lane's rows
        int32_t Ll[R];
        uint32_t code[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { Dl[r] = INF; Ll[r] = 0; code[r] = 0u; }
        // the cell above-left of column 0: the virtual origin (0, L = 0) for the very first row, +inf elsewhere
        Cell diag{(ps == 0 && t == 0) ? 0.0f : INF, 0};
        const int n_steps = Fb + t_last;
        __syncthreads();                                            // ring zero fill; the previous pass's last reads and bout stores
        for (int s = 0; s < n_steps; ++s) {
            if ((s & (NT - 1)) == 0 && s < Fb) {                    // refill the half nobody reads any more: chunk c = s / NT
                const int slot0 = s & NT;                           // (c & 1) * NT
                const int ncol = min(NT, Fb - s);
                const float* src = B + (size_t)s * n_coef;
                for (int e = t; e < ncol * n_coef; e += NT) {
                    const int col = e / n_coef;
                    ring[(slot0 + col) * STR + (e - col * n_coef)] = src[e];
                }
                if (t < ncol) top[slot0 + t] = ps == 0 ? Cell{INF, 0} : bin[s + t];
                __syncthreads();
            }
            const int j = s - t;
            const bool active = t <= t_last && j >= 0 && j < Fb;
            Cell best{INF, 0};
            if (active) {
                const Cell up_in = t == 0 ? top[j & (RING - 1)] : hand[((s - 1) & 1) * NT + t - 1];
                const float4* brow = reinterpret_cast<const float4*>(ring + (j & (RING - 1)) * STR);
                float acc[R];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll
                for (int q = 0; q < NC / 4; ++q) {
                    const float4 b4 = brow[q];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        float df = a[r][4 * q] - b4.x;     acc[r] = fmaf(df, df, acc[r]);
                        df = a[r][4 * q + 1] - b4.y;       acc[r] = fmaf(df, df, acc[r]);
                        df = a[r][4 * q + 2] - b4.z;       acc[r] = fmaf(df, df, acc[r]);
                        df = a[r][4 * q + 3] - b4.w;       acc[r] = fmaf(df, df, acc[r]);
                    }
                }
                Cell dg = diag, up = up_in;
                long long v = (long long)j * fa1 - (long long)i0 * fb1;      // band test: |j (Fa-1) - i (Fb-1)| <= w max(Fa-1, Fb-1)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float dist = scale * sqrtf(2.0f * acc[r]);
                    Cell b = dg;                                    // ties: diagonal, then up, then left
                    uint32_t c = 0u;
                    if (up.D < b.D) { b = up; c = 1u; }
                    if (Dl[r] < b.D) { b = Cell{Dl[r], Ll[r]}; c = 2u; }
                    Cell n{dist + b.D, b.L + 1};
                    if (limit >= 0 && (v < 0 ? -v : v) > limit) n = Cell{INF, 0};
                    v -= fb1;
                    dg = Cell{Dl[r], Ll[r]};                        // (i, j-1) is the diagonal of row i + 1
                    up = n;
                    Dl[r] = n.D; Ll[r] = n.L;
                    if (PATH) code[r] |= c << (2 * (j & 15));
                    if (last_pass && j == Fb - 1 && i0 + r == Fa - 1) {
                        total[p] = n.D;
                        path_len[p] = n.L;
                        mcd[p] = n.D / (float)n.L;
                    }
                }
                diag = up_in;
                best = up;                                          // this lane's last row at column j
                if (PATH && ((j & 15) == 15 || j == Fb - 1)) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (i0 + r < Fa) cw[(size_t)(i0 + r) * wpr + (j >> 4)] = code[r];
                        code[r] = 0u;
                    }
                }
                hand[(s & 1) * NT + t] = best;
                if (!last_pass && t == NT - 1) bout[j] = best;      // (only a full pass is followed by another)
            }
            __syncthreads();
        }
    }
}

// One workgroup of 64 lanes per pair.  Lane 0 walks the codes from the end cell and writes the path back to front
// (its length is known); then all lanes fill the rows beyond it with -1.  A pair whose total is not finite (a band
// that disconnects the end from the start) has no path: all -1.
__global__ void __launch_bounds__(64)
backtrack_kernel(const uint32_t* __restrict__ codes, int wpr, const int32_t* __restrict__ len_a,
                 const int32_t* __restrict__ len_b, const float* __restrict__ total, const int32_t* __restrict__ path_len,
                 int max_a, int max_b, int32_t* __restrict__ path) {
    const int p = blockIdx.x;
    const int rows = max_a + max_b - 1;
    int32_t* out = path + (size_t)p * rows * 2;
    const int Fa = min(max(len_a[p], 1), max_a);
    const int Fb = min(max(len_b[p], 1), max_b);
    int n = path_len[p];
    if (!(total[p] < __builtin_inff()) || n < 1 || n > Fa + Fb - 1) n = 0;
    if (threadIdx.x == 0 && n > 0) {
        const uint32_t* cw = codes + (size_t)p * max_a * wpr;
        int i = Fa - 1, j = Fb - 1;
        for (int k = n - 1; k >= 0; --k) {
            out[2 * k] = i;
            out[2 * k + 1] = j;
            if (i == 0 && j == 0) break;
            uint32_t c = (cw[(size_t)i * wpr + (j >> 4)] >> (2 * (j & 15))) & 3u;
            if (i == 0) c = 2u;                                     // the first row and column have one way back
            else if (j == 0) c = 1u;
            if (c != 2u) --i;
            if (c != 1u) --j;
        }
    }
    for (int k = n + (int)threadIdx.x; k < rows; k += 64) { out[2 * k] = -1; out[2 * k + 1] = -1; }
}

// Frame-synchronous score: mcd = (1 / n) sum_{i < n} d(i, i), n = min(Fa, Fb).  Lane t adds frames t, t + 256, ... in
// that order; the 256 partial sums are added in a fixed tree.
__global__ void __launch_bounds__(NT)
frame_mcd_kernel(const float* __restrict__ ca, const float* __restrict__ cb, const int32_t* __restrict__ len_a,
                 const int32_t* __restrict__ len_b, int max_a, int max_b, int n_coef, float scale, float* __restrict__ mcd) {
    __shared__ float part[NT];
    const int p = blockIdx.x;
    const int t = threadIdx.x;
    const int n = min(min(max(len_a[p], 1), max_a), min(max(len_b[p], 1), max_b));
    const float* __restrict__ A = ca + (size_t)p * max_a * n_coef;
    const float* __restrict__ B = cb + (size_t)p * max_b * n_coef;
    float sum = 0.0f;
    for (int i = t; i < n; i += NT) {
        float acc = 0.0f;
        for (int d = 0; d < n_coef; ++d) {
            const float df = A[(size_t)i * n_coef + d] - B[(size_t)i * n_coef + d];
            acc = fmaf(df, df, acc);
        }
        sum += scale * sqrtf(2.0f * acc);
    }
    part[t] = sum;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) mcd[p] = part[0] / (float)n;
}

// c[row, d] = sum_m dct[d, m] * mel[row, m], m ascending, fused multiply-adds.  The table sits transposed in LDS
// ([m][d]: the lanes of one row read consecutive words); the lanes that share a row read the same mel word.
template <typename T>
__global__ void __launch_bounds__(NT)
cepstra_kernel(const T* __restrict__ mel, long long rows, int n_mels, const float* __restrict__ dct, int n_coef,
               float* __restrict__ cep) {
    extern __shared__ __align__(16) float tabT[];                   // [n_mels][n_coef]
    for (int e = threadIdx.x; e < n_mels * n_coef; e += NT) {
        const int d = e / n_mels, m = e - d * n_mels;
        tabT[m * n_coef + d] = dct[e];
    }
    __syncthreads();
    const long long n_out = rows * n_coef;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n_out; e += (long long)gridDim.x * NT) {
        const long long row = e / n_coef;
        const int d = (int)(e - row * n_coef);
        const T* x = mel + row * n_mels;
        float acc = 0.0f;
        for (int m = 0; m < n_mels; ++m) acc = fmaf(tabT[m * n_coef + d], (float)x[m], acc);
        cep[e] = acc;
    }
}

template <int NC, bool PATH>
int launch_dtw(hipStream_t st, int batch, const float* ca, const float* cb, const int32_t* la, const int32_t* lb, int max_a,
               int max_b, int n_coef, float scale, int band, float* total, int32_t* plen, float* mcd, Cell* bound,
               uint32_t* codes, int wpr) {
    // more than 64 KB of LDS needs the attribute once per device and instantiation (a caller that captures a graph
    // makes its first call outside the capture, as with every large-LDS launch of this library)
    static std::mutex mu;
    static unsigned long long done = 0ull;                          // one bit per device ordinal
    int dev = 0;
    VC_HIP_CHECK(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= 64 || !((done >> dev) & 1ull)) {
            VC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(dtw_kernel<NC, PATH>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, dtw_lds_bytes<NC>()));
            if (dev < 64) done |= 1ull << dev;
        }
    }
    hipLaunchKernelGGL((dtw_kernel<NC, PATH>), dim3(batch), dim3(NT), (size_t)dtw_lds_bytes<NC>(), st, ca, cb, la, lb, max_a,
                       max_b, n_coef, scale, band, total, plen, mcd, bound, codes, wpr);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

bool dtw_shape_ok(int batch, int max_a, int max_b) {
    return batch >= 1 && batch <= 65535 && max_a >= 1 && max_a <= MAX_FRAMES && max_b >= 1 && max_b <= MAX_FRAMES;
}

long long code_bytes(int batch, int max_a, int max_b) { return (long long)batch * max_a * words_per_row(max_b) * 4; }

}  // namespace

extern "C" {

int vc_mel_cepstra(const void* d_mel, int32_t mel_dtype, int32_t rows, int32_t n_mels, const float* d_dct, int32_t n_coef,
                   float* d_cep, void* stream) {
    VC_REQUIRE(d_mel && d_dct && d_cep, "vc_mel_cepstra: NULL argument");
    VC_REQUIRE(mel_dtype == VC_F32 || mel_dtype == VC_BF16, "vc_mel_cepstra: mel_dtype must be VC_F32 or VC_BF16 (got %d)", mel_dtype);
    VC_REQUIRE(rows >= 1 && n_mels >= 1 && n_mels <= 512 && n_coef >= 1 && n_coef <= n_mels && n_coef <= MAX_COEF,
               "vc_mel_cepstra: bad shape (rows %d, n_mels %d, n_coef %d; need 1 <= n_coef <= min(n_mels, %d), n_mels <= 512)", rows,
               n_mels, n_coef, MAX_COEF);
    const long long n_out = (long long)rows * n_coef;
    const unsigned grid = (unsigned)((n_out + NT - 1) / NT < 4096 ? (n_out + NT - 1) / NT : 4096);
    const size_t lds = (size_t)n_mels * n_coef * sizeof(float);     // at most 64 KB
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mel_dtype == VC_F32)
        hipLaunchKernelGGL(cepstra_kernel<float>, dim3(grid), dim3(NT), lds, st, static_cast<const float*>(d_mel), (long long)rows,
                           n_mels, d_dct, n_coef, d_cep);
    else
        hipLaunchKernelGGL(cepstra_kernel<__bf16>, dim3(grid), dim3(NT), lds, st, static_cast<const __bf16*>(d_mel), (long long)rows,
                           n_mels, d_dct, n_coef, d_cep);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

size_t vc_dtw_workspace_size(int32_t batch, int32_t max_a, int32_t max_b, int32_t want_path) {
    if (!dtw_shape_ok(batch, max_a, max_b)) return 0;
    size_t need = boundary_bytes(batch, max_b);
    if (want_path) {
        if (code_bytes(batch, max_a, max_b) > MAX_CODE_BYTES) return 0;
        need += vc::align256((size_t)code_bytes(batch, max_a, max_b));
    }
    return need;
}

int vc_dtw_f32(const float* d_ca, const float* d_cb, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
               int32_t max_a, int32_t max_b, int32_t n_coef, float scale, int32_t band, int32_t want_path, float* d_total,
               int32_t* d_path_len, float* d_mcd, void* d_workspace, size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_ca && d_cb && d_len_a && d_len_b && d_total && d_path_len && d_mcd && d_workspace, "vc_dtw_f32: NULL argument");
    VC_REQUIRE(dtw_shape_ok(batch, max_a, max_b), "vc_dtw_f32: bad shape (batch %d, max_a %d, max_b %d; need 1 <= frames <= %d, "
               "batch <= 65535)", batch, max_a, max_b, MAX_FRAMES);
    VC_REQUIRE(n_coef >= 1 && std::isfinite(scale) && scale > 0.0f && band >= -1,
               "vc_dtw_f32: need n_coef >= 1, a finite scale > 0 and band >= -1 (-1: none); got %d, %g, %d", n_coef, (double)scale, band);
    if (n_coef > MAX_COEF)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_dtw_f32: n_coef %d exceeds the %d coefficients a lane keeps in registers", n_coef,
                             MAX_COEF);
    if (want_path && code_bytes(batch, max_a, max_b) > MAX_CODE_BYTES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_dtw_f32: the predecessor codes of %d pairs of %d x %d frames take %lld bytes, more "
                             "than the limit of %lld; score fewer pairs per call", batch, max_a, max_b, code_bytes(batch, max_a, max_b),
                             MAX_CODE_BYTES);
    VC_REQUIRE((reinterpret_cast<uintptr_t>(d_ca) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_cb) & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "vc_dtw_f32: unaligned pointer");
    const size_t need = vc_dtw_workspace_size(batch, max_a, max_b, want_path);
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_dtw_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Cell* bound = static_cast<Cell*>(d_workspace);
    uint32_t* codes = want_path ? reinterpret_cast<uint32_t*>(static_cast<char*>(d_workspace) + boundary_bytes(batch, max_b)) : nullptr;
    const int wpr = words_per_row(max_b);
#define VC_DTW_GO(NC)                                                                                                          \
    return want_path ? launch_dtw<NC, true>(st, batch, d_ca, d_cb, d_len_a, d_len_b, max_a, max_b, n_coef, scale, band, d_total, \
                                            d_path_len, d_mcd, bound, codes, wpr)                                              \
                     : launch_dtw<NC, false>(st, batch, d_ca, d_cb, d_len_a, d_len_b, max_a, max_b, n_coef, scale, band, d_total, \
                                             d_path_len, d_mcd, bound, codes, wpr)
    if (n_coef <= 8) { VC_DTW_GO(8); }
    if (n_coef <= 16) { VC_DTW_GO(16); }
    if (n_coef <= 24) { VC_DTW_GO(24); }
    VC_DTW_GO(32);
#undef VC_DTW_GO
}

int vc_dtw_backtrack(const void* d_workspace, size_t workspace_bytes, const int32_t* d_len_a, const int32_t* d_len_b,
                     const float* d_total, const int32_t* d_path_len, int32_t batch, int32_t max_a, int32_t max_b, int32_t* d_path,
                     void* stream) {
    VC_REQUIRE(d_workspace && d_len_a && d_len_b && d_total && d_path_len && d_path, "vc_dtw_backtrack: NULL argument");
    VC_REQUIRE(dtw_shape_ok(batch, max_a, max_b), "vc_dtw_backtrack: bad shape (batch %d, max_a %d, max_b %d)", batch, max_a, max_b);
    if (code_bytes(batch, max_a, max_b) > MAX_CODE_BYTES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_dtw_backtrack: %d pairs of %d x %d frames exceed the limit of %lld bytes of "
                             "predecessor codes", batch, max_a, max_b, MAX_CODE_BYTES);
    const size_t need = vc_dtw_workspace_size(batch, max_a, max_b, 1);
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_dtw_backtrack: workspace of %zu bytes, %zu needed (the one vc_dtw_f32 filled with "
                             "want_path)", workspace_bytes, need);
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(static_cast<const char*>(d_workspace) + boundary_bytes(batch, max_b));
    hipLaunchKernelGGL(backtrack_kernel, dim3(batch), dim3(64), 0, static_cast<hipStream_t>(stream), codes, words_per_row(max_b),
                       d_len_a, d_len_b, d_total, d_path_len, max_a, max_b, d_path);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_frame_mcd_f32(const float* d_ca, const float* d_cb, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
                     int32_t max_a, int32_t max_b, int32_t n_coef, float scale, float* d_mcd, void* stream) {
    VC_REQUIRE(d_ca && d_cb && d_len_a && d_len_b && d_mcd, "vc_frame_mcd_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && batch <= 65535 && max_a >= 1 && max_b >= 1 && n_coef >= 1 && std::isfinite(scale) && scale > 0.0f,
               "vc_frame_mcd_f32: bad shape (batch %d, max_a %d, max_b %d, n_coef %d) or scale %g", batch, max_a, max_b, n_coef,
               (double)scale);
    hipLaunchKernelGGL(frame_mcd_kernel, dim3(batch), dim3(NT), 0, static_cast<hipStream_t>(stream), d_ca, d_cb, d_len_a, d_len_b,
                       max_a, max_b, n_coef, scale, d_mcd);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
