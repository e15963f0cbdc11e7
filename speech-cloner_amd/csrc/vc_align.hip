// Forced alignment on the device (include/vc_hip.h, "Alignment"): where does each state of a KNOWN sequence lie in the
// frames of an utterance?  A left-to-right Viterbi pass over the given states with stay / advance / skip-an-optional-state
// moves, float32, one IEEE add and strict compare-selects per cell, and the boundaries read back from the stored moves.
//
//     e(t, s) = score[t, seq[s]]                       (-inf for a class outside [0, C))
//     D(t, s) = e(t, s) + best,  best = D(t-1, s), then D(t-1, s-1) iff strictly greater, then D(t-1, s-2) iff opt[s-1]
//                                and strictly greater                             (codes 0, 1, 2)
//
// align_forward_kernel<K>: the geometry of vc_lattice.h (state table, gather, neighbours, end read-out are its helpers;
// vc_fullsum.hip walks the same lattice): one workgroup of ONE wave per utterance.  Lane l owns the K consecutive states l K .. l K + K - 1,
// their D in registers.  A frame's step takes the left neighbour's last two D of the previous row by two shuffles BEFORE
// the lane overwrites its own, then updates its states from the highest down (D[k-1], D[k-2] are still the previous row's).
// No LDS, no barrier.  The K emissions of a frame are gathered AL_PF = 4 frames ahead into a register ring (the frame
// index is clamped to F - 1, so the loads are unconditional and their count per step is fixed); the frame loop is unrolled
// by 16, so ring slots and code shifts are compile-time.  The two-bit codes of 16 frames make one 32-bit word per state,
// stored once per 16 frames: codes[b][t / 16][s], bits 2 (t % 16).  States from S on carry -inf and are never stored.
//
// align_backtrack_kernel: a second launch, one workgroup of 256 lanes per utterance.  Lane 0 walks the codes from
// (F - 1, final) to frame 0 -- one load per (word, state) visited, not per frame -- and leaves first frame / one past the
// last frame of every visited state in LDS (initialised to -1 by all lanes first).  After the barrier lane s, s + 256, ...
// owns state s: it writes the boundaries, the state's index into its frames of frame_state, and the float64 sum of its
// emissions in frame order divided by the count, rounded once.  The rows of frame_state from F on are filled here too.
// Every output element is written exactly once; no atomics, no memset.
#include <cmath>
#include "vc_lattice.h"

namespace {

namespace lat = vc::lattice;
constexpr int AL_MAX_SEQ = lat::MAX_SEQ;
constexpr int AL_MAX_CLASSES = 65535;
constexpr int AL_PF = lat::PF;          // frames of emissions in flight
constexpr int AL_NT_B = 256;            // lanes of the back-track launch

__host__ __device__ inline size_t al_code_words(int max_frames) { return ((size_t)max_frames + 15) / 16; }

inline size_t al_ws_bytes(int batch, int max_frames, int max_seq) {
    return vc::align256((size_t)batch * sizeof(int32_t)) + vc::align256((size_t)batch * al_code_words(max_frames) * max_seq * sizeof(uint32_t));
}

template <int K>
__global__ void __launch_bounds__(64)
align_forward_kernel(const float* __restrict__ score, const int32_t* __restrict__ seq, const uint8_t* __restrict__ opt,
                     const int32_t* __restrict__ n_frames, const int32_t* __restrict__ n_seq, int max_frames, int max_seq,
                     int n_classes, float* __restrict__ total, int32_t* __restrict__ final_state, uint32_t* __restrict__ codes) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int F = __builtin_amdgcn_readfirstlane(min(max(n_frames[b], 0), max_frames));
    const int S = __builtin_amdgcn_readfirstlane(min(max(n_seq[b], 0), max_seq));
    const float ninf = -__builtin_inff();
    if (F == 0 || S == 0) {                                         // infeasible (uniform)
        if (lane == 0) { total[b] = ninf; final_state[b] = -1; }
        return;
    }
    const float* __restrict__ X = score + (size_t)b * max_frames * n_classes;
    const int32_t* __restrict__ Q = seq + (size_t)b * max_seq;
    const uint8_t* __restrict__ O = opt ? opt + (size_t)b * max_seq : nullptr;
    uint32_t* __restrict__ W = codes + (size_t)b * al_code_words(max_frames) * max_seq;
    const int s0 = lane * K;
    int cls[K];                         // the checked class of each state (0 where there is none)
    uint32_t valid, skip;               // bit k: state s0 + k has an emission / may be entered by a skip
    lat::state_table<K, false>(Q, O, S, s0, n_classes, cls, valid, skip);
    const bool opt0 = O && O[0] != 0;
    float D[K];
    float ring[AL_PF][K];
#pragma unroll
    for (int k = 0; k < K; ++k) D[k] = ninf;
#pragma unroll
    for (int p = 0; p < AL_PF; ++p) lat::gather<K>(X, min(p, F - 1), n_classes, cls, ring[p]);
    const int n_words = (F + 15) >> 4;
    for (int w = 0; w < n_words; ++w) {
        uint32_t cw[K];
#pragma unroll
        for (int k = 0; k < K; ++k) cw[k] = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int t = w * 16 + j;
            float e[K];
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = (valid >> k) & 1 ? ring[j % AL_PF][k] : ninf;
            lat::gather<K>(X, min(t + AL_PF, F - 1), n_classes, cls, ring[j % AL_PF]);
            if (t >= F) continue;                                   // (uniform; only in the last word)
            if (j == 0 && w == 0) {                                 // frame 0
#pragma unroll
                for (int k = 0; k < K; ++k) D[k] = (s0 + k == 0 || (s0 + k == 1 && opt0)) ? e[k] : ninf;
                continue;
            }
            // the left neighbour's last two states of the previous row, before this lane overwrites its own
            const lat::Two left = lat::left_two<K>(D, lane);
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {
                const float p1 = k >= 1 ? D[k >= 1 ? k - 1 : 0] : left.near;
                const float p2 = k >= 2 ? D[k >= 2 ? k - 2 : 0] : (k == 1 ? left.near : left.far);
                float best = D[k];
                uint32_t code = 0;
                if (p1 > best) { best = p1; code = 1; }
                if (((skip >> k) & 1) && p2 > best) { best = p2; code = 2; }
                D[k] = e[k] + best;
                cw[k] |= code << (2 * j);
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (s0 + k < S) W[(size_t)w * max_seq + s0 + k] = cw[k];
    }
    const lat::Two d_end = lat::end_two<K>(D, s0, S, O);            // D(F-1, S-1); D(F-1, S-2) if a path may end there
    int fin = S - 1;
    float tot = d_end.near;
    if (d_end.far > d_end.near) { fin = S - 2; tot = d_end.far; }
    if (lane == 0) { total[b] = tot; final_state[b] = tot == ninf ? -1 : fin; }
}

__global__ void __launch_bounds__(AL_NT_B)
align_backtrack_kernel(const float* __restrict__ score, const int32_t* __restrict__ seq, const int32_t* __restrict__ n_frames,
                       const int32_t* __restrict__ n_seq, int max_frames, int max_seq, int n_classes,
                       const int32_t* __restrict__ final_state, const uint32_t* __restrict__ codes, int32_t* __restrict__ frame_state,
                       int32_t* __restrict__ start, int32_t* __restrict__ end, float* __restrict__ seg_score,
                       int32_t* __restrict__ n_visited) {
    __shared__ int s_start[AL_MAX_SEQ], s_end[AL_MAX_SEQ];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int F = min(max(n_frames[b], 0), max_frames);
    const int S = min(max(n_seq[b], 0), max_seq);
    const int fin = final_state[b];
    const bool feasible = F > 0 && S > 0 && fin >= 0 && fin < S;
    const float* __restrict__ X = score + (size_t)b * max_frames * n_classes;
    const int32_t* __restrict__ Q = seq + (size_t)b * max_seq;
    const uint32_t* __restrict__ W = codes + (size_t)b * al_code_words(max_frames) * max_seq;
    int32_t* out_f = frame_state + (size_t)b * max_frames;
    for (int s = tid; s < max_seq; s += AL_NT_B) { s_start[s] = -1; s_end[s] = -1; }
    __syncthreads();
    if (tid == 0) {
        int nv = 0;
        if (feasible) {
            int s = fin, have_w = -1, have_s = -1;
            uint32_t word = 0;
            s_end[s] = F;
            nv = 1;
            for (int t = F - 1; t >= 1; --t) {
                const int w = t >> 4;
                if (w != have_w || s != have_s) { word = W[(size_t)w * max_seq + s]; have_w = w; have_s = s; }
                const int c = min(min((int)((word >> (2 * (t & 15))) & 3u), 2), s);      // (a code never leaves the lattice)
                if (c) {
                    s_start[s] = t;
                    s -= c;
                    s_end[s] = t;
                    ++nv;
                }
            }
            s_start[s] = 0;
        }
        n_visited[b] = nv;
    }
    __syncthreads();
    for (int s = tid; s < max_seq; s += AL_NT_B) {
        const int st = s_start[s], en = s_end[s];
        start[(size_t)b * max_seq + s] = st;
        end[(size_t)b * max_seq + s] = en;
        float mean = __builtin_nanf("");
        if (st >= 0) {
            const int c = Q[s];
            const bool ok = c >= 0 && c < n_classes;
            const float* __restrict__ col = X + (ok ? c : 0);
            double acc = 0.0;
            for (int t = st; t < en; ++t) {
                out_f[t] = s;
                acc += (double)(ok ? col[(size_t)t * n_classes] : -__builtin_inff());
            }
            mean = (float)(acc / (double)(en - st));
        }
        seg_score[(size_t)b * max_seq + s] = mean;
    }
    for (int t = (feasible ? F : 0) + tid; t < max_frames; t += AL_NT_B) out_f[t] = -1;
}

}  // namespace

extern "C" {

size_t vc_align_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_seq) {
    const size_t need = al_ws_bytes(batch, max_frames, max_seq);
    return lat::shape_ok(batch, max_frames, max_seq, need) ? need : 0;
}

int vc_align_f32(const float* d_score, const int32_t* d_seq, const uint8_t* d_opt, const int32_t* d_n_frames, const int32_t* d_n_seq,
                 int32_t batch, int32_t max_frames, int32_t max_seq, int32_t n_classes, int32_t* d_frame_state, int32_t* d_start,
                 int32_t* d_end, float* d_seg_score, float* d_total, int32_t* d_n_visited, void* d_workspace, size_t workspace_bytes,
                 void* stream) {
    const size_t need = al_ws_bytes(batch, max_frames, max_seq);
    if (int rc = lat::check_args("vc_align_f32", d_score && d_seq && d_n_frames && d_n_seq && d_frame_state && d_start && d_end &&
                                 d_seg_score && d_total && d_n_visited && d_workspace, batch, max_frames, max_seq, n_classes,
                                 AL_MAX_CLASSES, d_workspace, workspace_bytes, need))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* fin = static_cast<int32_t*>(d_workspace);
    uint32_t* codes = reinterpret_cast<uint32_t*>(static_cast<char*>(d_workspace) + vc::align256((size_t)batch * sizeof(int32_t)));
    lat::dispatch_per_lane(max_seq, [&](auto k) {
        hipLaunchKernelGGL(align_forward_kernel<decltype(k)::value>, dim3(batch), dim3(64), 0, st, d_score, d_seq, d_opt, d_n_frames,
                           d_n_seq, max_frames, max_seq, n_classes, d_total, fin, codes);
    });
    VC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(align_backtrack_kernel, dim3(batch), dim3(AL_NT_B), 0, st, d_score, d_seq, d_n_frames, d_n_seq, max_frames,
                       max_seq, n_classes, fin, codes, d_frame_state, d_start, d_end, d_seg_score, d_n_visited);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
