// Exemplar conversion (include/vc_hip.h, "Exemplar conversion"): int8 keys of posteriorgrams, the exact k-nearest-neighbour
// search over them on the int8 matrix cores, and the mean of the retrieved rows.  tests/exemplar_ref.py restates all three.
//
// The search.  One wave owns 16 queries for a whole sweep over its split of the bank.  v_mfma_i32_16x16x64_i8 takes a tile of
// 16 bank rows as A and the 16 queries as B; its C layout (col = lane & 15, row = 4 * (lane >> 4) + reg) hands every lane ONE
// query and four bank rows per instruction.  Lane l feeds bytes 16 * (l >> 4) .. + 15 of bank row l & 15 as A and the same
// bytes of query l & 15 as B: both operands cut K the same way, so whichever order the instruction walks a lane's 16 bytes
// in, the sum over K is the dot product (integer arithmetic: no order dependence).  The queries are negated once, so that
// the accumulator holds -dot and  nb + 2 * acc  (one v_lshl_add_u32) is the distance less the query's own norm, which is a
// constant of the lane and joins at the end.  A lane keeps its k best in registers, tests a tile's four values against its
// k-th best with one minimum and one compare, and takes the unrolled insertion only when that fails.  Within a lane the
// bank rows arrive in ascending order, so a value equal to a kept one never displaces it: the sweep compares distances
// alone.  The four lane groups of a query then merge their lists by (d, j) through two rounds of lane exchanges, and a
// second launch merges the splits: the first k of a union are the first k of the parts' first k.
#include <climits>
#include <cstdint>

#include "vc_common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int WAVES = 4;                 // query tiles per workgroup of the sweep
constexpr int EMPTY = 0x20000000;        // distance of a slot without a candidate; every real distance is below 2^22
constexpr int BARRED = 0x40000000;       // "norm" of a bank row that is no candidate: BARRED - 2 * 2,064,512 > EMPTY
constexpr int MAX_K = 16;
constexpr int MAX_SPLITS = 1024;
constexpr int MAX_ROWS = 1 << 24;

__host__ __device__ inline int list_len(int k) { return k <= 1 ? 1 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

__device__ __forceinline__ bool before(int d, int j, int d2, int j2) { return d < d2 || (d == d2 && j < j2); }

// (d, j) into a list sorted by (d, j); the caller has found it before the last entry.
template <int KT>
__device__ __forceinline__ void insert_pair(int (&ld)[KT], int (&lj)[KT], int d, int j) {
#pragma unroll
    for (int i = KT - 1; i >= 1; --i) {
        const bool shift = before(d, j, ld[i - 1], lj[i - 1]);
        const bool here = before(d, j, ld[i], lj[i]);
        ld[i] = shift ? ld[i - 1] : (here ? d : ld[i]);
        lj[i] = shift ? lj[i - 1] : (here ? j : lj[i]);
    }
    if (before(d, j, ld[0], lj[0])) { ld[0] = d; lj[0] = j; }
}

// The sweep's insertion: j exceeds every j of the list, so the order is that of d with the newcomer last among equals.
template <int KT>
__device__ __forceinline__ void insert_last(int (&ld)[KT], int (&lj)[KT], int d, int j) {
#pragma unroll
    for (int i = KT - 1; i >= 1; --i) {
        const bool shift = d < ld[i - 1];
        const bool here = d < ld[i];
        ld[i] = shift ? ld[i - 1] : (here ? d : ld[i]);
        lj[i] = shift ? lj[i - 1] : (here ? j : lj[i]);
    }
    if (d < ld[0]) { ld[0] = d; lj[0] = j; }
}

// ------------------------------------------------------------------------------------------------------------------- keys
__global__ __launch_bounds__(256) void ppg_key_kernel(const float* __restrict__ ppg, const int32_t* __restrict__ n_frames, int rows,
                                                      int max_frames, int C, int Kp, int8_t* __restrict__ key,
                                                      int32_t* __restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                          // (a whole wave)
    const int b = row / max_frames, f = row - b * max_frames;
    const bool live = f < n_frames[b];
    int sq = 0;
    for (int c = lane; c < Kp; c += 64) {
        int q = 0;
        if (live && c < C) {
            const float p = ppg[(size_t)row * C + c];
            // sqrtf, not __fsqrt_rn: the intrinsic is the 1-ulp native root here, sqrtf the correctly rounded one
            if (p > 0.0f) q = (int)fminf(127.0f, rintf(127.0f * sqrtf(p)));
        }
        key[(size_t)row * Kp + c] = (int8_t)q;
        sq += q * q;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sq += __shfl_xor(sq, s, 64);
    if (lane == 0) norm[row] = sq;
}

// ----------------------------------------------------------------------------------------------------------------- search
struct KnnArgs {
    const int8_t* qkey;
    const int32_t* qnorm;
    const int32_t* n_frames;
    const int32_t* excl;
    const int8_t* bkey;
    const int32_t* bnorm;
    int Mq, max_frames, N, n_splits;
    int2* ws;
};

// -x in every byte of a word whose bytes lie in [0, 127]
__device__ __forceinline__ int neg_bytes(int w) { return (int)((0x80808080u - (unsigned)w) ^ 0x80808080u); }

template <int KT, int KP>
__global__ __launch_bounds__(64 * WAVES) void knn_sweep_kernel(KnnArgs a) {
    const int lane = threadIdx.x & 63;
    const int qt = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (qt >= (a.Mq + 15) >> 4) return;                               // (a whole wave; the kernel has no barrier)
    const int split = blockIdx.y;
    const int col = lane & 15, g = lane >> 4;
    const int m = qt * 16 + col;
    const int mc = min(m, a.Mq - 1);
    const int b = mc / a.max_frames, f = mc - b * a.max_frames;
    const bool live = m < a.Mq && f < a.n_frames[b];

    // the queries, negated, for the whole sweep
    v4i q0 = *reinterpret_cast<const v4i*>(a.qkey + (size_t)mc * KP + 16 * g), q1 = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) q0[i] = neg_bytes(q0[i]);
    if (KP == 128) {
        q1 = *reinterpret_cast<const v4i*>(a.qkey + (size_t)mc * KP + 64 + 16 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) q1[i] = neg_bytes(q1[i]);
    }
    // the lane's exclusion, and the span that holds every lane's
    int e0 = 0, e1 = 0;
    if (a.excl) { e0 = a.excl[2 * b]; e1 = a.excl[2 * b + 1]; }
    int lo = e1 > e0 ? e0 : INT_MAX, hi = e1 > e0 ? e1 : 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo = min(lo, __shfl_xor(lo, s, 64));
        hi = max(hi, __shfl_xor(hi, s, 64));
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);

    int ld[KT], lj[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) { ld[i] = EMPTY; lj[i] = -1; }
    int worst = live ? EMPTY : INT_MIN;                               // a dead query takes nothing

    const int tiles = (a.N + 15) >> 4;
    const int t0 = (int)((long long)split * tiles / a.n_splits), t1 = (int)((long long)(split + 1) * tiles / a.n_splits);
    const int8_t* arow = a.bkey + 16 * g;
    for (int t = t0; t < t1; ++t) {
        const int r0 = t * 16;
        const int ra = min(r0 + col, a.N - 1);
        const v4i A0 = *reinterpret_cast<const v4i*>(arow + (size_t)ra * KP);
        v4i acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0, q0, acc, 0, 0, 0);
        if (KP == 128) {
            const v4i A1 = *reinterpret_cast<const v4i*>(arow + (size_t)ra * KP + 64);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, q1, acc, 0, 0, 0);
        }
        const int j0 = r0 + 4 * g;
        v4i nb;
        if (r0 + 16 <= a.N && !(r0 < hi && r0 + 16 > lo)) {           // (uniform) a whole tile that no lane excludes from
            nb = *reinterpret_cast<const v4i*>(a.bnorm + j0);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + r;
                nb[r] = (j < a.N && !(j >= e0 && j < e1)) ? a.bnorm[j] : BARRED;
            }
        }
        int d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = (acc[r] << 1) + nb[r];
        if (min(min(d[0], d[1]), min(d[2], d[3])) < worst) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (d[r] < worst) {
                    insert_last<KT>(ld, lj, d[r], j0 + r);
                    worst = ld[KT - 1];
                }
        }
    }

    // the four lane groups of a query: lanes col, col + 16, col + 32, col + 48
#pragma unroll
    for (int s = 16; s <= 32; s <<= 1) {
        int od[KT], oj[KT];
#pragma unroll
        for (int i = 0; i < KT; ++i) { od[i] = __shfl_xor(ld[i], s, 64); oj[i] = __shfl_xor(lj[i], s, 64); }
#pragma unroll
        for (int i = 0; i < KT; ++i)
            if (before(od[i], oj[i], ld[KT - 1], lj[KT - 1])) insert_pair<KT>(ld, lj, od[i], oj[i]);
    }
    if (g == 0 && m < a.Mq) {
        const int nq = a.qnorm[m];
        int2* out = a.ws + ((size_t)split * a.Mq + m) * KT;
#pragma unroll
        for (int i = 0; i < KT; ++i) out[i] = make_int2(ld[i] < EMPTY ? ld[i] + nq : EMPTY, lj[i]);
    }
}

template <int KT>
__global__ __launch_bounds__(64) void knn_merge_kernel(const int2* __restrict__ ws, int n_splits, int Mq, int k, int32_t* __restrict__ idx,
                                                       int32_t* __restrict__ dist) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= Mq) return;
    int ld[KT], lj[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) { ld[i] = EMPTY; lj[i] = -1; }
    for (int s = 0; s < n_splits; ++s) {
        const int2* in = ws + ((size_t)s * Mq + m) * KT;
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const int2 e = in[i];
            if (e.x < EMPTY && before(e.x, e.y, ld[KT - 1], lj[KT - 1])) insert_pair<KT>(ld, lj, e.x, e.y);
        }
    }
#pragma unroll
    for (int i = 0; i < KT; ++i)
        if (i < k) {
            const bool filled = ld[i] < EMPTY;
            idx[(size_t)m * k + i] = filled ? lj[i] : -1;
            dist[(size_t)m * k + i] = filled ? ld[i] : -1;
        }
}

// ------------------------------------------------------------------------------------------------------------------- mean
__global__ __launch_bounds__(256) void knn_mean_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ dist, int Mq, int k,
                                                       int d_max, const float* __restrict__ V, int N, int D, float* __restrict__ out,
                                                       int32_t* __restrict__ n_used) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= Mq) return;
    int rows[MAX_K];
    int n = 0;
#pragma unroll
    for (int i = 0; i < MAX_K; ++i) {
        rows[i] = 0;
        if (i < k && n == i) {                                        // (uniform) the list ends at the first slot that fails
            const int j = idx[(size_t)m * k + i];
            if (j >= 0 && j < N && (i == 0 || d_max < 0 || dist[(size_t)m * k + i] <= d_max)) { rows[i] = j; n = i + 1; }
        }
    }
    if (lane == 0) n_used[m] = n;
    const float fn = (float)n;
    for (int c = lane; c < D; c += 64) {
        float s = 0.0f;
        if (n > 0) {
            s = V[(size_t)rows[0] * D + c];
#pragma unroll
            for (int i = 1; i < MAX_K; ++i)
                if (i < n) s = s + V[(size_t)rows[i] * D + c];
            s = s / fn;
        }
        out[(size_t)m * D + c] = s;
    }
}

int auto_splits(int Mq, int N) {
    // enough waves to fill 256 CUs x 4 SIMDs eight deep, while a split still sweeps 32 tiles or more
    const int q_tiles = (Mq + 15) / 16, tiles = (N + 15) / 16;
    int n = (8192 + q_tiles - 1) / q_tiles;
    n = n < tiles / 32 ? n : tiles / 32;
    n = n < 256 ? n : 256;
    return n < 1 ? 1 : n;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int KT>
void launch_search(const KnnArgs& a, int KP, int k, int32_t* idx, int32_t* dist, hipStream_t st) {
    const dim3 grid((unsigned)(((a.Mq + 15) / 16 + WAVES - 1) / WAVES), (unsigned)a.n_splits);
    if (KP == 64)
        hipLaunchKernelGGL((knn_sweep_kernel<KT, 64>), grid, dim3(64 * WAVES), 0, st, a);
    else
        hipLaunchKernelGGL((knn_sweep_kernel<KT, 128>), grid, dim3(64 * WAVES), 0, st, a);
    hipLaunchKernelGGL((knn_merge_kernel<KT>), dim3((unsigned)((a.Mq + 63) / 64)), dim3(64), 0, st, (const int2*)a.ws, a.n_splits, a.Mq, k,
                       idx, dist);
}

}  // namespace

extern "C" {

int32_t vc_knn_key_width(int32_t n_classes) { return n_classes < 1 || n_classes > 128 ? 0 : n_classes <= 64 ? 64 : 128; }

int vc_ppg_key_i8(const float* d_ppg, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_classes, int8_t* d_key,
                  int32_t* d_norm, void* stream) {
    const char* fn = "vc_ppg_key_i8";
    VC_REQUIRE(d_ppg && d_n_frames && d_key && d_norm, "%s: NULL argument", fn);
    VC_REQUIRE(n_classes >= 1 && n_classes <= 128, "%s: n_classes must be in [1, 128] (got %d)", fn, n_classes);
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && (long long)batch * max_frames <= MAX_ROWS,
               "%s: batch %d and max_frames %d must be positive with at most 2^24 rows", fn, batch, max_frames);
    const int rows = batch * max_frames;
    hipLaunchKernelGGL(ppg_key_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_ppg, d_n_frames, rows,
                       max_frames, n_classes, vc_knn_key_width(n_classes), d_key, d_norm);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int32_t vc_knn_splits(int32_t n_queries, int32_t n_bank, int32_t n_splits) {
    if (n_queries < 1 || n_queries > MAX_ROWS || n_bank < 1 || n_bank > MAX_ROWS || n_splits < 0 || n_splits > MAX_SPLITS) return 0;
    return n_splits ? n_splits : auto_splits(n_queries, n_bank);
}

size_t vc_knn_workspace_bytes(int32_t n_queries, int32_t n_bank, int32_t k, int32_t n_splits) {
    const int n = vc_knn_splits(n_queries, n_bank, n_splits);
    if (!n || k < 1 || k > MAX_K) return 0;
    return (size_t)n * n_queries * list_len(k) * sizeof(int2);
}

int vc_knn_i8(const int8_t* d_qkey, const int32_t* d_qnorm, const int32_t* d_n_frames, const int32_t* h_excl, const int32_t* d_excl,
              int32_t batch, int32_t max_frames, const int8_t* d_bkey, const int32_t* d_bnorm, int32_t n_bank, int32_t key_width,
              int32_t k, int32_t n_splits, void* d_workspace, size_t workspace_bytes, int32_t* d_idx, int32_t* d_dist, void* stream) {
    const char* fn = "vc_knn_i8";
    VC_REQUIRE(d_qkey && d_qnorm && d_n_frames && d_bkey && d_bnorm && d_workspace && d_idx && d_dist, "%s: NULL argument", fn);
    VC_REQUIRE((h_excl == nullptr) == (d_excl == nullptr), "%s: pass the exclusion table's host and device copies together or neither",
               fn);
    VC_REQUIRE(k >= 1 && k <= MAX_K, "%s: k must be in [1, %d] (got %d)", fn, MAX_K, k);
    VC_REQUIRE(key_width == 64 || key_width == 128, "%s: key_width must be 64 or 128 (got %d)", fn, key_width);
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && (long long)batch * max_frames <= MAX_ROWS,
               "%s: batch %d and max_frames %d must be positive with at most 2^24 query rows", fn, batch, max_frames);
    VC_REQUIRE(n_bank >= 1 && n_bank <= MAX_ROWS, "%s: n_bank must be in [1, 2^24] (got %d)", fn, n_bank);
    VC_REQUIRE(n_splits >= 0 && n_splits <= MAX_SPLITS, "%s: n_splits must be in [0, %d] (got %d)", fn, MAX_SPLITS, n_splits);
    VC_REQUIRE(aligned16(d_qkey) && aligned16(d_bkey) && aligned16(d_bnorm) && aligned16(d_workspace),
               "%s: the keys, the bank's norms and the workspace must be 16-byte aligned", fn);
    if (h_excl)
        for (int b = 0; b < batch; ++b)
            VC_REQUIRE(h_excl[2 * b] >= 0 && h_excl[2 * b] <= h_excl[2 * b + 1] && h_excl[2 * b + 1] <= n_bank,
                       "%s: excl[%d] = (%d, %d) must be ordered and inside [0, %d]", fn, b, h_excl[2 * b], h_excl[2 * b + 1], n_bank);
    const int Mq = batch * max_frames;
    const size_t need = vc_knn_workspace_bytes(Mq, n_bank, k, n_splits);
    if (workspace_bytes < need) return vc::set_error(VC_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    KnnArgs a;
    a.qkey = d_qkey; a.qnorm = d_qnorm; a.n_frames = d_n_frames; a.excl = d_excl; a.bkey = d_bkey; a.bnorm = d_bnorm;
    a.Mq = Mq; a.max_frames = max_frames; a.N = n_bank; a.n_splits = vc_knn_splits(Mq, n_bank, n_splits);
    a.ws = static_cast<int2*>(d_workspace);
    const hipStream_t st = (hipStream_t)stream;
    switch (list_len(k)) {
        case 1: launch_search<1>(a, key_width, k, d_idx, d_dist, st); break;
        case 4: launch_search<4>(a, key_width, k, d_idx, d_dist, st); break;
        case 8: launch_search<8>(a, key_width, k, d_idx, d_dist, st); break;
        default: launch_search<16>(a, key_width, k, d_idx, d_dist, st); break;
    }
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_knn_mean_f32(const int32_t* d_idx, const int32_t* d_dist, int32_t n_queries, int32_t k, int32_t d_max, const float* d_values,
                    int32_t n_bank, int32_t dim, float* d_out, int32_t* d_n_used, void* stream) {
    const char* fn = "vc_knn_mean_f32";
    VC_REQUIRE(d_idx && d_dist && d_values && d_out && d_n_used, "%s: NULL argument", fn);
    VC_REQUIRE(k >= 1 && k <= MAX_K, "%s: k must be in [1, %d] (got %d)", fn, MAX_K, k);
    VC_REQUIRE(n_queries >= 1 && n_queries <= MAX_ROWS, "%s: n_queries must be in [1, 2^24] (got %d)", fn, n_queries);
    VC_REQUIRE(n_bank >= 1 && n_bank <= MAX_ROWS, "%s: n_bank must be in [1, 2^24] (got %d)", fn, n_bank);
    VC_REQUIRE(dim >= 1 && dim <= 65536, "%s: dim must be in [1, 65536] (got %d)", fn, dim);
    hipLaunchKernelGGL(knn_mean_kernel, dim3((unsigned)((n_queries + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_idx, d_dist, n_queries, k,
                       d_max, d_values, n_bank, dim, d_out, d_n_used);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
