// Full-sum alignment on the device (include/vc_hip.h, "Alignment", second half): the DISTRIBUTION over the paths of a known
// sequence through the frames, where vc_align.hip gives the best one.  Forward-backward on the same lattice (stay /
// advance / skip one optional state), float32 log domain, each frame's row shifted by its own maximum:
//
//     e(t, s)  = score[t, seq[s]]                        (-inf for a class outside [0, C))
//     la(t, s) = e(t, s) + lse(la(t-1, s), la(t-1, s-1), [opt[s-1]] la(t-1, s-2))
//     lb(t, s) = lse(lb(t+1, s) + e(t+1, s), lb(t+1, s+1) + e(t+1, s+1), [opt[s+1]] lb(t+1, s+2) + e(t+1, s+2))
//     gamma(t, s) = exp(la + lb - log_z),  Gamma(t, c) = sum of gamma(t, s) over seq[s] = c,  occ(s) = sum_t gamma(t, s)
//
// fullsum_forward_kernel<K>: the geometry of vc_lattice.h, shared with align_forward_kernel<K> -- one workgroup of ONE
// wave per utterance, lane l owns the K consecutive states l K .. l K + K - 1, the left neighbour's last two values come by
// two shuffles before the lane overwrites its own, the K emissions of a frame are gathered FS_PF = 4 frames ahead (frame index clamped to F - 1)
// into a register ring, the frame loop is unrolled by FS_PF so that ring slots are compile-time.  After each frame the
// row's maximum over the states (a wave reduction) is subtracted and added to a float64 sum; the shifted row A(t, .) goes
// to the workspace [batch, max_frames, max_seq] (states below S only).  log_z = (sum of the shifts) + lse of the last
// row's end states, rounded once.  A row that is all -inf is left as it is (no -inf - -inf anywhere).
//
// fullsum_backward_kernel<K>: the same geometry, time reversed, lb in registers, the right neighbour's first two values by
// two shuffles.  The row is shifted by its maximum too (no sum is kept: nothing needs it).  gamma is formed from the
// stored row and NORMALISED over the states of the frame -- exp(A + B - max) / sum, the sum one binary tree over the state
// index, the same tree for every K -- which is the definition (the sum over s of exp(la + lb) is Z at every frame) without
// the shifts, so neither the shifts nor log_z enter gamma.  gamma goes out when asked for, is added to the owning lane's
// occ, and is added into the frame's Gamma row in LDS as a 2^-30 fixed-point integer (ds_add_u32: integer addition
// commutes, so the arrival order of several states of one class cannot change a bit; a row sums to 1, so the word cannot
// overflow).  The row is then written out coalesced -- zeros for the absent classes included -- and cleared by the lanes
// that read it.  Rows from F on, the columns from S on and an infeasible utterance (log_z = -inf, read back from the forward
// launch) are zero-filled here; every output element is written exactly once.
#include <cmath>
#include "vc_lattice.h"

namespace {

namespace lat = vc::lattice;
constexpr int FS_MAX_CLASSES = 4096;    // the Gamma row in LDS: 16 KiB of 32-bit words
constexpr int FS_PF = lat::PF;          // frames of emissions (and of stored rows) in flight
constexpr float FS_FIX = 1073741824.0f; // 2^30

inline size_t fs_ws_bytes(int batch, int max_frames, int max_seq) {
    return vc::align256((size_t)batch * max_frames * max_seq * sizeof(float));
}

// The sum of a row of 64 K values, lane l holding the K consecutive ones from l K on, as ONE balanced binary tree over the
// state index: pairs, then pairs of pairs, inside the lane and on across the lanes -- neighbours, quads (after which a
// quad's lanes agree, so the half mirror pairs quad with quad), eights, rows of 16, then row 0 + 1 and 2 + 3, then the two
// halves, read from lane 63 (vc::wave_sum: what it leaves in lane 63 is this tree).  The tree over the states of an utterance is the same for every K -- a larger K only adds
// levels that add zeros -- so the sum is too.
template <int K>
__device__ __forceinline__ float fs_row_sum(const float (&p)[K]) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = p[k];
#pragma unroll
    for (int w = 1; w < K; w <<= 1)
#pragma unroll
        for (int k = 0; k < K; k += 2 * w) v[k] += v[k + w];
    return vc::wave_sum(v[0]);
}

// log(exp(x0) + exp(x1) + exp(x2)) for finite or -inf arguments; -inf when all three are
__device__ __forceinline__ float fs_lse3(float x0, float x1, float x2) {
    const float m = fmaxf(x0, fmaxf(x1, x2));
    if (m == -__builtin_inff()) return m;
    return m + __logf(__expf(x0 - m) + __expf(x1 - m) + __expf(x2 - m));
}

template <int K>
__global__ void __launch_bounds__(64)
fullsum_forward_kernel(const float* __restrict__ score, const int32_t* __restrict__ seq, const uint8_t* __restrict__ opt,
                       const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_seq, int max_frames, int max_seq,
                       int n_classes, float* __restrict__ log_z, float* __restrict__ rows) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int F = __builtin_amdgcn_readfirstlane(min(max(n_frames[b], 0), max_frames));
    const int S = __builtin_amdgcn_readfirstlane(min(max(n_seq[b], 0), max_seq));
    const float ninf = -__builtin_inff();
    if (F == 0 || S == 0) {                                         // infeasible (uniform)
        if (lane == 0) log_z[b] = ninf;
        return;
    }
    const float* __restrict__ X = score + (size_t)b * max_frames * n_classes;
    const int32_t* __restrict__ Q = seq + (size_t)b * max_seq;
    const uint8_t* __restrict__ O = opt ? opt + (size_t)b * max_seq : nullptr;
    float* __restrict__ W = rows + (size_t)b * max_frames * max_seq;
    const int s0 = lane * K;
    int cls[K];                         // the checked class of each state (0 where there is none)
    uint32_t valid, skip;               // bit k: state s0 + k has an emission / may be entered by a skip
    lat::state_table<K, false>(Q, O, S, s0, n_classes, cls, valid, skip);
    const bool opt0 = O && O[0] != 0;
    float A[K];
    float ring[FS_PF][K];
#pragma unroll
    for (int k = 0; k < K; ++k) A[k] = ninf;
#pragma unroll
    for (int p = 0; p < FS_PF; ++p) lat::gather<K>(X, min(p, F - 1), n_classes, cls, ring[p]);
    double shift_sum = 0.0;
    for (int t0 = 0; t0 < F; t0 += FS_PF) {
#pragma unroll
        for (int j = 0; j < FS_PF; ++j) {
            const int t = t0 + j;
            float e[K];
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = (valid >> k) & 1 ? ring[j][k] : ninf;
            lat::gather<K>(X, min(t + FS_PF, F - 1), n_classes, cls, ring[j]);
            if (t >= F) continue;                                   // (uniform; only in the last group)
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) A[k] = (s0 + k == 0 || (s0 + k == 1 && opt0)) ? e[k] : ninf;
            } else {
                // the left neighbour's last two states of the previous row, before this lane overwrites its own
                const lat::Two left = lat::left_two<K>(A, lane);
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {
                    const float p1 = k >= 1 ? A[k >= 1 ? k - 1 : 0] : left.near;
                    const float p2 = k >= 2 ? A[k >= 2 ? k - 2 : 0] : (k == 1 ? left.near : left.far);
                    A[k] = e[k] + fs_lse3(A[k], p1, ((skip >> k) & 1) ? p2 : ninf);
                }
            }
            float m = ninf;
#pragma unroll
            for (int k = 0; k < K; ++k) m = fmaxf(m, A[k]);
            m = vc::wave_max_inf(m);
            if (m != ninf) {                                        // (uniform)
                shift_sum += (double)m;
#pragma unroll
                for (int k = 0; k < K; ++k) A[k] -= m;
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (s0 + k < S) W[(size_t)t * max_seq + s0 + k] = A[k];
        }
    }
    const lat::Two a_end = lat::end_two<K>(A, s0, S, O);            // A(F-1, S-1); A(F-1, S-2) if a path may end there
    const float rel = fs_lse3(a_end.near, a_end.far, ninf);
    if (lane == 0) log_z[b] = rel == ninf ? ninf : (float)(shift_sum + (double)rel);
}

template <int K>
__global__ void __launch_bounds__(64)
fullsum_backward_kernel(const float* __restrict__ score, const int32_t* __restrict__ seq, const uint8_t* __restrict__ opt,
                        const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_seq, int max_frames, int max_seq,
                        int n_classes, const float* __restrict__ log_z, const float* __restrict__ rows,
                        float* __restrict__ class_post, float* __restrict__ state_post, float* __restrict__ occ) {
    __shared__ uint32_t s_row[FS_MAX_CLASSES];
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const float ninf = -__builtin_inff();
    const int S = __builtin_amdgcn_readfirstlane(min(max(n_seq[b], 0), max_seq));
    int F = __builtin_amdgcn_readfirstlane(min(max(n_frames[b], 0), max_frames));
    if (S == 0 || __builtin_amdgcn_readfirstlane(log_z[b] == ninf ? 1 : 0)) F = 0;      // infeasible: zeros everywhere
    const float* __restrict__ X = score + (size_t)b * max_frames * n_classes;
    const int32_t* __restrict__ Q = seq + (size_t)b * max_seq;
    const uint8_t* __restrict__ O = opt ? opt + (size_t)b * max_seq : nullptr;
    const float* __restrict__ W = rows + (size_t)b * max_frames * max_seq;
    float* __restrict__ G = class_post + (size_t)b * max_frames * n_classes;
    float* __restrict__ P = state_post ? state_post + (size_t)b * max_frames * max_seq : nullptr;
    const int s0 = lane * K;
    float acc[K];                       // occ of the lane's states, frames added from the last to the first
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0f;
    if (F > 0) {
        int cls[K], col[K];             // the checked class / the clamped column of the stored row
        uint32_t valid, skip, live, last;       // bit k: has an emission / may be LEFT by a skip / s < S / end state
        lat::state_table<K, true>(Q, O, S, s0, n_classes, cls, valid, skip);
        lat::state_table_ends<K>(O, S, s0, col, live, last);
        for (int c = lane; c < n_classes; c += 64) s_row[c] = 0;
        __syncthreads();
        float B[K], e1[K];              // lb of frame t + 1 (then t), shifted; the emissions of frame t + 1
        float ring_e[FS_PF][K], ring_a[FS_PF][K];
#pragma unroll
        for (int k = 0; k < K; ++k) { B[k] = ninf; e1[k] = ninf; }
#pragma unroll
        for (int p = 0; p < FS_PF; ++p) {
            lat::gather<K>(X, max(F - 1 - p, 0), n_classes, cls, ring_e[p]);
            lat::gather<K>(W, max(F - 1 - p, 0), max_seq, col, ring_a[p]);
        }
        for (int i0 = 0; i0 < F; i0 += FS_PF) {
#pragma unroll
            for (int j = 0; j < FS_PF; ++j) {
                const int t = F - 1 - i0 - j;
                float e[K], a[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    e[k] = (valid >> k) & 1 ? ring_e[j][k] : ninf;
                    a[k] = (live >> k) & 1 ? ring_a[j][k] : ninf;
                }
                lat::gather<K>(X, max(t - FS_PF, 0), n_classes, cls, ring_e[j]);
                lat::gather<K>(W, max(t - FS_PF, 0), max_seq, col, ring_a[j]);
                if (t < 0) continue;                                // (uniform; only in the last group)
                if (t == F - 1) {
#pragma unroll
                    for (int k = 0; k < K; ++k) B[k] = (last >> k) & 1 ? 0.0f : ninf;
                } else {
                    float g[K];                                     // lb(t+1, s) + e(t+1, s): -inf from S on
#pragma unroll
                    for (int k = 0; k < K; ++k) g[k] = B[k] + e1[k];
                    const lat::Two right = lat::right_two<K>(g, lane);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float n1 = k + 1 < K ? g[k + 1 < K ? k + 1 : 0] : right.near;
                        const float n2 = k + 2 < K ? g[k + 2 < K ? k + 2 : 0] : (k + 2 == K ? right.near : right.far);
                        B[k] = fs_lse3(g[k], n1, ((skip >> k) & 1) ? n2 : ninf);
                    }
                    float m = ninf;
#pragma unroll
                    for (int k = 0; k < K; ++k) m = fmaxf(m, B[k]);
                    m = vc::wave_max_inf(m);
                    if (m != ninf) {                                // (uniform)
#pragma unroll
                        for (int k = 0; k < K; ++k) B[k] -= m;
                    }
                }
#pragma unroll
                for (int k = 0; k < K; ++k) e1[k] = e[k];
                // gamma of the frame: exp(A + B - max) over its sum
                float v[K], top = ninf;
#pragma unroll
                for (int k = 0; k < K; ++k) { v[k] = a[k] + B[k]; top = fmaxf(top, v[k]); }
                top = vc::wave_max_inf(top);
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] = top != ninf ? __expf(v[k] - top) : 0.0f;
                const float sum = fs_row_sum<K>(v);
                const float inv = sum > 0.0f ? __builtin_amdgcn_rcpf(sum) : 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float gam = v[k] * inv;
                    acc[k] += gam;
                    if (P && s0 + k < max_seq) P[(size_t)t * max_seq + s0 + k] = gam;
                    const uint32_t q = (uint32_t)__float2uint_rn(gam * FS_FIX);
                    if (q) atomicAdd(&s_row[cls[k]], q);            // (q != 0 only for a live state with a checked class)
                }
                __syncthreads();
                for (int c = lane; c < n_classes; c += 64) {
                    const uint32_t q = s_row[c];
                    s_row[c] = 0;
                    G[(size_t)t * n_classes + c] = (float)q * (1.0f / FS_FIX);
                }
                __syncthreads();
            }
        }
    }
    // what lies outside the utterance
    for (size_t i = (size_t)F * n_classes + lane, n = (size_t)max_frames * n_classes; i < n; i += 64) G[i] = 0.0f;
    if (P)
        for (size_t i = (size_t)F * max_seq + lane, n = (size_t)max_frames * max_seq; i < n; i += 64) P[i] = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (s0 + k < max_seq) occ[(size_t)b * max_seq + s0 + k] = acc[k];
}

}  // namespace

extern "C" {

size_t vc_fullsum_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_seq) {
    const size_t need = fs_ws_bytes(batch, max_frames, max_seq);
    return lat::shape_ok(batch, max_frames, max_seq, need) ? need : 0;
}

int vc_fullsum_f32(const float* d_score, const int32_t* d_seq, const uint8_t* d_opt, const int32_t* d_n_frames, const int32_t* d_n_seq,
                   int32_t batch, int32_t max_frames, int32_t max_seq, int32_t n_classes, float* d_log_z, float* d_class_post,
                   float* d_state_post, float* d_occ, void* d_workspace, size_t workspace_bytes, void* stream) {
    const size_t need = fs_ws_bytes(batch, max_frames, max_seq);
    if (int rc = lat::check_args("vc_fullsum_f32", d_score && d_seq && d_n_frames && d_n_seq && d_log_z && d_class_post && d_occ &&
                                 d_workspace, batch, max_frames, max_seq, n_classes, FS_MAX_CLASSES, d_workspace, workspace_bytes, need))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* rows = static_cast<float*>(d_workspace);
    lat::dispatch_per_lane(max_seq, [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(fullsum_forward_kernel<K>, dim3(batch), dim3(64), 0, st, d_score, d_seq, d_opt, d_n_frames, d_n_seq,
                           max_frames, max_seq, n_classes, d_log_z, rows);
        hipLaunchKernelGGL(fullsum_backward_kernel<K>, dim3(batch), dim3(64), 0, st, d_score, d_seq, d_opt, d_n_frames, d_n_seq,
                           max_frames, max_seq, n_classes, d_log_z, rows, d_class_post, d_state_post, d_occ);
    });
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
