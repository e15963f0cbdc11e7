// Pitch tracking on the device (include/vc_hip.h, "Pitch tracking"): the Viterbi decoding of a lattice of F0 candidates
// (csrc/vc_f0.hip, f0_candidates_kernel) with an unvoiced state.
//
//     S = n_cand + 1 <= 16 states: 0 unvoiced (local cost unvoiced_cost), k >= 1 candidate k - 1 (local cost cost[k - 1])
//     t(i, j) = 0 (both unvoiced), switch_cost (one of them), jump_cost * |pitch_i - pitch_j| (both voiced)
//     delta_f(j) = min_i (delta_{f-1}(i) + t(i, j)) + c_f(j), lowest i among equals; then m_f = min_j delta_f(j) is
//     subtracted from every state and added into a float64 total
//
// f0_viterbi_kernel: one wave per utterance; the recurrence is sequential over frames.  Lane l owns state l & 15 and the
// four predecessors 4 (l >> 4) .. + 3: the sixteen delta of the frame before go through sixteen words of LDS (one
// ds_write_b32, one ds_read_b128), each lane takes the best of its four in ascending order with a strict compare, and two
// (cost, index) exchanges with lanes l ^ 16 and l ^ 32 finish the state (the lower index wins a tie).  m_f is a minimum
// over a row of sixteen lanes on DPP.  The sixteen 4-bit back-pointers of a frame are four ballots (bit plane p of the
// sixteen indices in bits 16 p .. 16 p + 15 of one 64-bit word), kept in LDS and flushed to the workspace tile by tile.
// The lattice is staged in LDS a tile of VT frames at a time as a flat copy, two buffers: tile k + 1 is loaded into
// registers before the frames of tile k run and stored to the other buffer after them, so the frame loop reads LDS only
// (the other buffer also holds frame f - 1 when f opens a tile).  Then the same wave walks back tile by tile: the
// back-pointers of a tile into LDS, the walk in LDS, state and f0 of the tile stored by all lanes.  Every output
// element is written exactly once; no atomics, no memset; float32 additions and products are not contracted.
#include <cmath>
#include "vc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_CAND = 15;
constexpr int NS = 16;                  // states
constexpr int VT = 128;                 // frames per staging tile (vc_f0_viterbi_tile)
constexpr int LAT = VT * MAX_CAND;      // floats of a tile's pitch or cost at most
constexpr int PF = LAT / 64;            // of them per lane
constexpr int MAX_FRAMES_V = (1 << 30) + 1;

__device__ __forceinline__ float row16_min(float v) {
    const float inf = __builtin_inff();
    v = fminf(v, vc::dpp_move<0xB1, 0xF>(inf, v));                  // quad_perm [1,0,3,2]
    v = fminf(v, vc::dpp_move<0x4E, 0xF>(inf, v));                  // quad_perm [2,3,0,1]
    v = fminf(v, vc::dpp_move<0x141, 0xF>(inf, v));                 // row_half_mirror
    v = fminf(v, vc::dpp_move<0x140, 0xF>(inf, v));                 // row_mirror: every lane of a row of 16
    return v;
}

__global__ void __launch_bounds__(64)
f0_viterbi_kernel(const float* __restrict__ pitch, const float* __restrict__ cost, const int32_t* __restrict__ n_in,
                  const int32_t* __restrict__ lens, int max_frames, int nc, float uc, float jc, float sc,
                  const float* __restrict__ cand_f0, unsigned long long* __restrict__ ws, int32_t* __restrict__ state,
                  float* __restrict__ f0, float* __restrict__ total) {
    __shared__ __align__(16) float lp[2][LAT];
    __shared__ __align__(16) float lc[2][LAT];
    __shared__ int ln[2][VT];
    __shared__ __align__(16) float dx[NS];
    __shared__ unsigned long long bp[VT];
    __shared__ int st[VT];
    const int l = threadIdx.x, j = l & 15, g = l >> 4, b = blockIdx.x;
    const float inf = __builtin_inff();
    const int F = lens ? min(max(lens[b], 0), max_frames) : max_frames;
    const size_t row = (size_t)b * max_frames;
    const float* __restrict__ P = pitch + row * nc;
    const float* __restrict__ C = cost + row * nc;
    const int32_t* __restrict__ N = n_in + row;
    unsigned long long* __restrict__ Wb = ws + row;
    const int n_tiles = (F + VT - 1) / VT;
    float rp[PF], rc[PF];
    int rn[VT / 64];

#define VIT_LOAD(k)                                                                                   \
    {                                                                                                 \
        const int fr = min(F - (k) * VT, VT), cnt = fr * nc;                                          \
        const size_t base = (size_t)(k) * VT * nc;                                                    \
        _Pragma("unroll") for (int u = 0; u < PF; ++u) {                                              \
            const int e = l + 64 * u;                                                                 \
            rp[u] = e < cnt ? P[base + e] : 0.0f;                                                     \
            rc[u] = e < cnt ? C[base + e] : 0.0f;                                                     \
        }                                                                                             \
        _Pragma("unroll") for (int u = 0; u < VT / 64; ++u) {                                         \
            const int e = l + 64 * u;                                                                 \
            rn[u] = e < fr ? N[(k) * VT + e] : 0;                                                     \
        }                                                                                             \
    }
#define VIT_STORE(k)                                                                                  \
    {                                                                                                 \
        _Pragma("unroll") for (int u = 0; u < PF; ++u) {                                              \
            lp[(k) & 1][l + 64 * u] = rp[u];                                                          \
            lc[(k) & 1][l + 64 * u] = rc[u];                                                          \
        }                                                                                             \
        _Pragma("unroll") for (int u = 0; u < VT / 64; ++u) ln[(k) & 1][l + 64 * u] = rn[u];          \
    }

    if (n_tiles > 0) {
        VIT_LOAD(0)
        VIT_STORE(0)
    }
    __syncthreads();
    float delta = inf;                                              // delta of state j after the frame before, less its minimum
    int np = 0;                                                     // candidates of the frame before
    double tot = 0.0;
    for (int k = 0; k < n_tiles; ++k) {
        if (k + 1 < n_tiles) VIT_LOAD(k + 1)
        const int buf = k & 1, f_lo = k * VT, f_hi = min(F, f_lo + VT);
        for (int f = f_lo; f < f_hi; ++f) {
            const int r = f - f_lo;
            const int nf = min(max(ln[buf][r], 0), nc);
            // every lane reads a slot that exists (its own, or slot 0 for the unvoiced state): what an absent state reads
            // is discarded below, so no read waits on a comparison
            const int mine = r * nc + max(j - 1, 0);
            const float cv = lc[buf][mine], pj = lp[buf][mine];
            const float cj = j == 0 ? uc : (j <= nf ? cv : inf);
            float d = cj;
            int bi = 0;
            if (f > 0) {                                            // uniform
                const float* pp = &lp[((f - 1) / VT) & 1][((f - 1) % VT) * nc];
                if (l < NS) dx[l] = delta;
                float pi[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) pi[q] = pp[max(4 * g + q - 1, 0)];
                __syncthreads();
                const float4 dv = *reinterpret_cast<const float4*>(&dx[4 * g]);
                const float dq[4] = {dv.x, dv.y, dv.z, dv.w};
                float best = inf;
                bi = 4 * g;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = 4 * g + q;
                    float t = jc * fabsf(pi[q] - pj);
                    if (i == 0 || j == 0) t = (i == 0 && j == 0) ? 0.0f : sc;
                    const float cand = i <= np ? dq[q] + t : inf;   // an absent predecessor, whatever its slot holds
                    if (cand < best) { best = cand; bi = i; }
                }
#pragma unroll
                for (int s = 16; s <= 32; s <<= 1) {
                    const float ob = __shfl_xor(best, s, 64);
                    const int oi = __shfl_xor(bi, s, 64);
                    const bool take = ob < best || (ob == best && oi < bi);
                    best = take ? ob : best;
                    bi = take ? oi : bi;
                }
                d = best + cj;
                __syncthreads();                                    // dx is written again by the next frame
            }
            np = nf;
            const float m = row16_min(d);                           // finite: state 0 is always there
            delta = d - m;
            tot += (double)m;
            unsigned long long w = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) w |= (__ballot((bi >> p) & 1) & 0xFFFFull) << (16 * p);
            if (l == 0) bp[r] = w;
        }
        __syncthreads();
        for (int e = l; e < f_hi - f_lo; e += 64) Wb[f_lo + e] = bp[e];
        if (k + 1 < n_tiles) VIT_STORE(k + 1)
        __syncthreads();
    }
#undef VIT_LOAD
#undef VIT_STORE
    // the last frame's state: the lowest j of minimal delta (zero after the subtraction)
    int s = 0;
    if (F > 0) s = __ffsll((long long)(__ballot(delta == 0.0f) & 0xFFFFull)) - 1;
    for (int k = n_tiles - 1; k >= 0; --k) {
        const int f_lo = k * VT, f_hi = min(F, f_lo + VT);
        __syncthreads();                                            // this wave's own stores above; st and bp of the tile after
        for (int e = l; e < f_hi - f_lo; e += 64) bp[e] = Wb[f_lo + e];
        __syncthreads();
        for (int r = f_hi - f_lo - 1; r >= 0; --r) {                // the same walk in every lane
            if (l == 0) st[r] = s;
            const unsigned long long w = bp[r] >> s;
            s = (int)((w & 1ull) | ((w >> 15) & 2ull) | ((w >> 30) & 4ull) | ((w >> 45) & 8ull));
        }
        __syncthreads();
        for (int e = l; e < f_hi - f_lo; e += 64) {
            const int sv = st[e];
            state[row + f_lo + e] = sv;
            if (f0) f0[row + f_lo + e] = sv > 0 ? cand_f0[(row + f_lo + e) * nc + min(sv, nc) - 1] : 0.0f;
        }
    }
    for (int f = F + l; f < max_frames; f += 64) {
        state[row + f] = -1;
        if (f0) f0[row + f] = 0.0f;
    }
    if (l == 0) total[b] = (float)tot;
}

}  // namespace

extern "C" {

int32_t vc_f0_viterbi_tile(void) { return VT; }

size_t vc_f0_viterbi_workspace_size(int32_t batch, int32_t max_frames, int32_t n_cand) {
    if (batch < 1 || batch > 65535 || max_frames < 1 || max_frames > MAX_FRAMES_V || n_cand < 1 || n_cand > MAX_CAND) return 0;
    return (size_t)batch * (size_t)max_frames * sizeof(unsigned long long);
}

int vc_f0_viterbi_f32(const float* d_pitch, const float* d_cost, const int32_t* d_n, const int32_t* d_frames, int32_t batch,
                      int32_t max_frames, int32_t n_cand, float unvoiced_cost, float jump_cost, float switch_cost,
                      const float* d_cand_f0, int32_t* d_state, float* d_f0, float* d_total, void* d_workspace,
                      size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_pitch && d_cost && d_n && d_state && d_total && d_workspace, "vc_f0_viterbi_f32: NULL argument");
    VC_REQUIRE((d_cand_f0 == nullptr) == (d_f0 == nullptr), "vc_f0_viterbi_f32: pass d_cand_f0 and d_f0 together, or NULL for both");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_cand >= 1, "vc_f0_viterbi_f32: bad shape (batch %d, max_frames %d, n_cand %d; need all "
               ">= 1)", batch, max_frames, n_cand);
    VC_REQUIRE(std::isfinite(unvoiced_cost) && unvoiced_cost >= 0.0f && std::isfinite(jump_cost) && jump_cost >= 0.0f &&
               std::isfinite(switch_cost) && switch_cost >= 0.0f,
               "vc_f0_viterbi_f32: unvoiced_cost, jump_cost and switch_cost must be finite and not negative (got %g, %g, %g)",
               (double)unvoiced_cost, (double)jump_cost, (double)switch_cost);
    const size_t need = vc_f0_viterbi_workspace_size(batch, max_frames, n_cand);
    if (need == 0)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_f0_viterbi_f32: limits are batch <= 65535, max_frames <= %d, n_cand <= %d; got batch "
                             "%d, max_frames %d, n_cand %d", MAX_FRAMES_V, MAX_CAND, batch, max_frames, n_cand);
    VC_REQUIRE(workspace_bytes >= need, "vc_f0_viterbi_f32: workspace of %zu bytes, need %zu (vc_f0_viterbi_workspace_size)",
               workspace_bytes, need);
    VC_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "vc_f0_viterbi_f32: the workspace must be 8-byte aligned");
    hipLaunchKernelGGL(f0_viterbi_kernel, dim3(batch), dim3(64), 0, static_cast<hipStream_t>(stream), d_pitch, d_cost, d_n, d_frames,
                       max_frames, n_cand, unvoiced_cost, jump_cost, switch_cost, d_cand_f0,
                       static_cast<unsigned long long*>(d_workspace), d_state, d_f0, d_total);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
