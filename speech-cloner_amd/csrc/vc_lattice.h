// The transcript lattice of vc_align.hip and vc_fullsum.hip, defined once: a KNOWN state sequence walked left to right
// with stay / advance / skip-one-optional-state moves, one wave per utterance, lane l owning the K consecutive states
// l K .. l K + K - 1 (K = 1, 2, 4, 8, 16 by the longest sequence of the batch).  Here are the parts that ARE the lattice
// -- which state has which emission, which may be skipped, what a lane needs from its neighbours, where a path may end --
// and the host side that both entry points share.  The frame loops, the recurrences (compare-select, lse3) and the
// storage stay with the kernels.
#pragma once
#include <type_traits>
#include "vc_device.h"

namespace vc::lattice {

constexpr int MAX_SEQ = 1024;           // 64 lanes of 16 states
constexpr int MAX_BATCH = 65535;
constexpr size_t MAX_WS = (size_t)1 << 31;
constexpr int PF = 4;                   // frames of emissions in flight

inline bool shape_ok(int batch, int max_frames, int max_seq, size_t ws_bytes) {
    return batch >= 1 && batch <= MAX_BATCH && max_frames >= 1 && max_seq >= 1 && max_seq <= MAX_SEQ && ws_bytes < MAX_WS;
}

// Calls f with the states per lane that max_seq needs, as a std::integral_constant: `[&](auto k) { kernel<k()> ... }`.
template <class F>
void dispatch_per_lane(int max_seq, F&& f) {
    const int per_lane = (max_seq + 63) / 64;
    if (per_lane <= 1) f(std::integral_constant<int, 1>{});
    else if (per_lane <= 2) f(std::integral_constant<int, 2>{});
    else if (per_lane <= 4) f(std::integral_constant<int, 4>{});
    else if (per_lane <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

// The checks both entry points make, in their order; `pointers` says whether every required pointer is there, `need` is
// the caller's workspace size for the shape.  VC_OK or the error, with `fn` leading the message.
inline int check_args(const char* fn, bool pointers, int batch, int max_frames, int max_seq, int n_classes, int max_classes,
                      const void* d_workspace, size_t workspace_bytes, size_t need) {
    if (!pointers) return vc::set_error(VC_ERR_INVALID, "%s: NULL argument", fn);
    if (!(batch >= 1 && max_frames >= 1 && max_seq >= 1 && n_classes >= 1))
        return vc::set_error(VC_ERR_INVALID, "%s: bad shape (batch %d, max_frames %d, max_seq %d, n_classes %d; need all >= 1)", fn,
                             batch, max_frames, max_seq, n_classes);
    if (n_classes > max_classes || !shape_ok(batch, max_frames, max_seq, need))
        return vc::set_error(VC_ERR_UNSUPPORTED, "%s: limits are batch <= %d, max_seq <= %d, n_classes <= %d and a workspace below "
                             "2 GiB; got batch %d, max_frames %d, max_seq %d, n_classes %d", fn, MAX_BATCH, MAX_SEQ, max_classes, batch,
                             max_frames, max_seq, n_classes);
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 3) != 0) return vc::set_error(VC_ERR_INVALID, "%s: unaligned workspace", fn);
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return VC_OK;
}

#if defined(__HIPCC__)
struct Two { float near, far; };        // two values by distance: from the lane's own states, or from the last state

// Where a path may end: S - 1, and S - 2 too iff the last state is optional.
__device__ __forceinline__ bool two_ends(const uint8_t* O, int S) { return S >= 2 && O && O[S - 1] != 0; }

// The state table of a lane: the checked class of each of its states (0 where there is none: past S, or a class outside
// [0, C), whose emission is -inf); bit k of `valid`: state s0 + k has an emission; bit k of `skip`: walking forward, the
// state may be ENTERED by a skip (over the optional s0 + k - 1), walking backward, it may be LEFT by one (over s0 + k + 1).
template <int K, bool BACKWARD>
__device__ __forceinline__ void state_table(const int32_t* __restrict__ Q, const uint8_t* __restrict__ O, int S, int s0,
                                            int n_classes, int (&cls)[K], uint32_t& valid, uint32_t& skip) {
    valid = 0;
    skip = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = s0 + k;
        const int c = s < S ? Q[s] : -1;
        const bool ok = c >= 0 && c < n_classes;
        cls[k] = ok ? c : 0;
        valid |= (ok ? 1u : 0u) << k;
        const bool over = BACKWARD ? O && s + 2 < S && O[s + 1] != 0 : O && s >= 2 && s < S && O[s - 1] != 0;
        skip |= (over ? 1u : 0u) << k;
    }
}

// What the backward walk needs besides.  Bit k of `live`: s0 + k < S; of `last`: a path may end there.  col: the state's
// column of a stored row, clamped into it.
template <int K>
__device__ __forceinline__ void state_table_ends(const uint8_t* __restrict__ O, int S, int s0, int (&col)[K], uint32_t& live,
                                                 uint32_t& last) {
    const bool two = two_ends(O, S);
    live = 0;
    last = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = s0 + k;
        col[k] = min(s, S - 1);
        live |= (s < S ? 1u : 0u) << k;
        last |= ((s == S - 1 || (two && s == S - 2)) ? 1u : 0u) << k;
    }
}

// One ring slot: the lane's K columns of row t of a [., width] matrix.  t is already clamped into the utterance, so the
// loads are unconditional and their count per step is fixed.
template <int K>
__device__ __forceinline__ void gather(const float* __restrict__ M, int t, int width, const int (&idx)[K], float (&slot)[K]) {
    const float* __restrict__ row = M + (size_t)t * width;
#pragma unroll
    for (int k = 0; k < K; ++k) slot[k] = row[idx[k]];
}

// The left neighbour's last two values (states s0 - 1 and s0 - 2), -inf where the lattice has none.  Call it before the
// lane overwrites its own.
template <int K>
__device__ __forceinline__ Two left_two(const float (&D)[K], int lane) {
    const float ninf = -__builtin_inff();
    float l1 = __shfl_up(D[K - 1], 1, 64);
    float l2 = K >= 2 ? __shfl_up(D[K >= 2 ? K - 2 : 0], 1, 64) : __shfl_up(D[0], 2, 64);
    if (lane == 0) { l1 = ninf; l2 = ninf; }
    if (K == 1 && lane == 1) l2 = ninf;
    return {l1, l2};
}

// The right neighbour's first two values (states s0 + K and s0 + K + 1), -inf where the lattice has none.
template <int K>
__device__ __forceinline__ Two right_two(const float (&D)[K], int lane) {
    const float ninf = -__builtin_inff();
    float r1 = __shfl_down(D[0], 1, 64);
    float r2 = K >= 2 ? __shfl_down(D[K >= 2 ? 1 : 0], 1, 64) : __shfl_down(D[0], 2, 64);
    if (lane == 63) { r1 = ninf; r2 = ninf; }
    if (K == 1 && lane == 62) r2 = ninf;
    return {r1, r2};
}

// The last row's values at the end states, in every lane: near at S - 1, far at S - 2 where a path may end there too
// (two_ends), else -inf.
template <int K>
__device__ __forceinline__ Two end_two(const float (&D)[K], int s0, int S, const uint8_t* O) {
    float d_last = -__builtin_inff(), d_prev = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (s0 + k == S - 1) d_last = D[k];
        if (s0 + k == S - 2) d_prev = D[k];
    }
    d_last = __shfl(d_last, (S - 1) / K, 64);
    d_prev = __shfl(d_prev, S >= 2 ? (S - 2) / K : 0, 64);
    return {d_last, two_ends(O, S) ? d_prev : -__builtin_inff()};
}
#endif

}  // namespace vc::lattice
