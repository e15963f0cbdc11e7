// Phoneme recognition on the device (include/vc_hip.h, "Decoding"): the best path through a LOOP of all classes, with a
// transition score between segments and a minimum duration of M frames per segment.  States (c, d), d = 0 .. M-1; float32,
// one IEEE add per term and strict compare-selects, and the path read back from one byte of moves per (frame, class).
//
//     X(t, c)        = max over i ascending of D(t-1, (i, M-1)) + trans[i, c], the lowest i on a tie: bp(t, c)
//     D(t, (c, 0))   = e(t, c) + X(t, c)                      (M = 1: e + best of stay, then enter iff strictly greater)
//     D(t, (c, d))   = e(t, c) + D(t-1, (c, d-1))             0 < d < M-1
//     D(t, (c, M-1)) = e(t, c) + best, best = stay, then advance from d = M-2 iff strictly greater
//
// decode_forward_kernel<NW>: one workgroup of NW waves per utterance, lane c owns destination class c.  Its eight D
// registers hold the states right-aligned: D[7] is (c, M-1), D[8 - M] is (c, 0), the ones below stay -inf, so the shift
// chain has compile-time indices for every M.  Per frame a lane needs the previous row's D(., M-1) of ALL classes and
// column c of trans:
//   NW = 1 (C <= 64)   the column lives in 64 registers; the row comes by v_readlane of lane i with constant i; no LDS, no
//                      barrier.
//   NW = 2 (C <= 128)  trans lives in LDS ([C][C], 64 KiB at 128 classes: lanes read consecutive words of row i), the row
//                      goes through two LDS buffers used in turn, ONE barrier per frame.
// The maximum over i runs as four independent chains over the four contiguous quarters of i, merged in ascending order
// with the same strict compare, which is the sequential rule (a later i wins only when strictly greater).  Emission
// rows are fetched DC_PF = 4 frames ahead with the frame index clamped to F - 1.  The move bytes of four frames make one
// 32-bit word per class, moves[b][c][t / 4], byte t % 4: bits 0-6 bp, bit 7 advance (enter when M = 1).  The column-major
// layout is for the walker, whose reads of one class are then consecutive bytes.
//
// decode_backtrack_kernel: one workgroup of 256 lanes per utterance.  Wave 0 walks: in class c at frame t its 64 lanes
// read the bytes (t, c), (t-1, c), ... and a ballot finds the first advance, so the walk costs one dependent step per
// segment (plus one per 64 frames of a long segment), not per frame; the predecessor's class is the bp byte at the
// segment's first frame, which is usually already in a lane of the same read.  The frames' classes go to LDS.  Then the
// whole block derives the outputs from them: a segment of the result is a maximal run of mapped labels (mapping, then
// merging equal neighbours, then dropping -1 leaves exactly the runs of class_map[frame_class] that are not -1), so each
// lane takes a contiguous chunk of frames, counts the kept run starts and run ends in it, one block scan gives the
// segment index of both, and a lane per segment adds its emissions in float64 in frame order.  The scan was chosen over a
// serial lane because a serial lane would pass over every frame once more (16,384 dependent LDS reads at the limit);
// the scan costs eight steps whatever F is.  Every output element is written exactly once; no atomics, no memset.
#include <cmath>
#include "vc_device.h"

namespace {

constexpr int DC_MAX_CLASSES = 128;
constexpr int DC_MAX_DUR = 8;
constexpr int DC_MAX_FRAMES = 16384;
constexpr int DC_PF = 4;                // frames of emissions in flight = frames per word of moves
constexpr int DC_NT_B = 256;            // lanes of the back-track launch
constexpr size_t DC_MAX_WS = (size_t)1 << 31;
constexpr int DC_FWD_LDS = DC_MAX_CLASSES * DC_MAX_CLASSES * 4 + 2 * 128 * 4;
constexpr int DC_BT_LDS = DC_MAX_FRAMES * 5;

__host__ __device__ inline size_t dc_words(int max_frames) { return ((size_t)max_frames + DC_PF - 1) / DC_PF; }

inline size_t dc_ws_bytes(int batch, int max_frames, int n_classes) {
    return vc::align256((size_t)batch * sizeof(int32_t)) + vc::align256((size_t)batch * n_classes * dc_words(max_frames) * sizeof(uint32_t));
}

inline bool dc_shape_ok(int batch, int max_frames, int n_classes) {
    if (batch < 1 || batch > 65535 || max_frames < 1 || max_frames > DC_MAX_FRAMES || n_classes < 1 || n_classes > DC_MAX_CLASSES) return false;
    return dc_ws_bytes(batch, max_frames, n_classes) < DC_MAX_WS;
}

__device__ __forceinline__ float dc_lane(float v, int lane) {      // lane: a compile-time constant after unrolling
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int NW>
__global__ void __launch_bounds__(64 * NW)
decode_forward_kernel(const float* __restrict__ score, const int32_t* __restrict__ n_frames, const float* __restrict__ trans,
                      const float* __restrict__ init, const float* __restrict__ fin_w, int max_frames, int C, int M,
                      float* __restrict__ total, int32_t* __restrict__ fin, uint32_t* __restrict__ moves) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // NW = 2: trans [C][C], then the row twice [2][128]
    const int b = blockIdx.x;
    const int c = threadIdx.x;
    const int F = __builtin_amdgcn_readfirstlane(min(max(n_frames[b], 0), max_frames));
    const float ninf = -__builtin_inff();
    if (F < M) {                                                    // infeasible (uniform; covers F = 0)
        if (c == 0) { total[b] = ninf; fin[b] = -1; }
        return;
    }
    const bool valid = c < C;
    const int cc = valid ? c : 0;
    const float* __restrict__ E = score + (size_t)b * max_frames * C + cc;
    uint32_t* __restrict__ W = moves + ((size_t)b * C + cc) * dc_words(max_frames);
    float tc[NW == 1 ? 64 : 1];
    float* const T = lds;
    float* const row = lds + (NW == 1 ? 0 : C * C);
    if constexpr (NW == 1) {
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const float v = trans[(size_t)min(i, C - 1) * C + cc];
            tc[i] = (valid && i < C) ? v : ninf;
        }
    } else {
        for (int k = c; k < C * C; k += 64 * NW) T[k] = trans[k];
    }
    float ring[DC_PF];
#pragma unroll
    for (int p = 0; p < DC_PF; ++p) ring[p] = E[(size_t)min(p, F - 1) * C];
    float D[DC_MAX_DUR];
#pragma unroll
    for (int k = 0; k < DC_MAX_DUR; ++k) D[k] = ninf;
    const int k0 = DC_MAX_DUR - M;                                  // the register of state (c, 0)
    int buf = 0;
    const int n_words = (F + DC_PF - 1) / DC_PF;
    for (int w = 0; w < n_words; ++w) {
        uint32_t cw = 0;
#pragma unroll
        for (int j = 0; j < DC_PF; ++j) {
            const int t = w * DC_PF + j;
            const float e = valid ? ring[j] : ninf;
            ring[j] = E[(size_t)min(t + DC_PF, F - 1) * C];
            if (t >= F) continue;                                   // (uniform; only in the last word)
            if (t == 0) {
                const float d0 = init ? init[cc] + e : e;
#pragma unroll
                for (int k = 0; k < DC_MAX_DUR; ++k) D[k] = k == k0 ? d0 : ninf;
                continue;
            }
            const float last = D[DC_MAX_DUR - 1];
            float xb[4];
            int xi[4];
            float x;
            int bp;
            if constexpr (NW == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { xb[q] = dc_lane(last, 16 * q) + tc[16 * q]; xi[q] = 16 * q; }
#pragma unroll
                for (int r = 1; r < 16; ++r) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float term = dc_lane(last, 16 * q + r) + tc[16 * q + r];
                        if (term > xb[q]) { xb[q] = term; xi[q] = 16 * q + r; }
                    }
                }
                x = xb[0]; bp = xi[0];
#pragma unroll
                for (int q = 1; q < 4; ++q)
                    if (xb[q] > x) { x = xb[q]; bp = xi[q]; }
            } else {
                float* const R = row + buf * 128;
                buf ^= 1;
                R[c] = last;
                __syncthreads();
                const int Q = C >> 2;                               // four chains of Q, then up to three tail classes
#pragma unroll
                for (int q = 0; q < 4; ++q) { xb[q] = R[q * Q] + T[q * Q * C + cc]; xi[q] = q * Q; }
                for (int r = 1; r < Q; ++r) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int i = q * Q + r;
                        const float term = R[i] + T[i * C + cc];
                        if (term > xb[q]) { xb[q] = term; xi[q] = i; }
                    }
                }
                x = xb[0]; bp = xi[0];
#pragma unroll
                for (int q = 1; q < 4; ++q)
                    if (xb[q] > x) { x = xb[q]; bp = xi[q]; }
                for (int i = 4 * Q; i < C; ++i) {
                    const float term = R[i] + T[i * C + cc];
                    if (term > x) { x = term; bp = i; }
                }
            }
            const float cand = M == 1 ? x : D[DC_MAX_DUR - 2];      // enter (M = 1) or advance, against stay
            const bool second = cand > last;
            const float top = e + (second ? cand : last);
#pragma unroll
            for (int k = DC_MAX_DUR - 2; k >= 1; --k) D[k] = e + (k == k0 ? x : D[k - 1]);
            D[0] = k0 == 0 ? e + x : ninf;
            D[DC_MAX_DUR - 1] = top;
            cw |= ((uint32_t)bp | (second ? 128u : 0u)) << (8 * j);
        }
        if (valid) W[w] = cw;
    }
    // the end: the greatest D(F-1, (c, M-1)) + final[c], the lowest class on a tie
    float v = valid ? (fin_w ? D[DC_MAX_DUR - 1] + fin_w[cc] : D[DC_MAX_DUR - 1]) : ninf;
    int vi = c;
    if constexpr (NW == 2) {
        float* const R = row + buf * 128;
        R[c] = v;
        __syncthreads();
        if (c >= 64) return;
        const float o = R[c + 64];
        if (o > v) { v = o; vi = c + 64; }
    }
    const vc::ArgMax top = vc::wave_argmax_low(v, vi);
    if (c == 0) { total[b] = top.v; fin[b] = top.v == ninf ? -1 : top.idx; }
}

__global__ void __launch_bounds__(DC_NT_B)
decode_backtrack_kernel(const float* __restrict__ score, const int32_t* __restrict__ n_frames, const int32_t* __restrict__ class_map,
                        int max_frames, int C, int M, const int32_t* __restrict__ fin, const uint32_t* __restrict__ moves,
                        int32_t* __restrict__ frame_class, int32_t* __restrict__ seg_label, int32_t* __restrict__ seg_start,
                        int32_t* __restrict__ seg_end, int32_t* __restrict__ n_seg, float* __restrict__ seg_score) {
    extern __shared__ __attribute__((aligned(16))) uint8_t bt_lds[];        // [max_frames] x (start u16, end u16, class u8)
    __shared__ int s_map[DC_MAX_CLASSES];
    __shared__ uint32_t s_scan[2][DC_NT_B];
    uint16_t* const s_st = reinterpret_cast<uint16_t*>(bt_lds);
    uint16_t* const s_en = s_st + max_frames;
    uint8_t* const s_fc = reinterpret_cast<uint8_t*>(s_en + max_frames);
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int F = min(max(n_frames[b], 0), max_frames);
    const int last = fin[b];
    const bool feasible = F >= M && last >= 0 && last < C;
    const int Fe = feasible ? F : 0;
    const size_t stride = dc_words(max_frames) * 4;                 // bytes of moves per class
    const uint8_t* __restrict__ Mv = reinterpret_cast<const uint8_t*>(moves) + (size_t)b * C * stride;
    const float* __restrict__ E = score + (size_t)b * max_frames * C;
    for (int k = tid; k < C; k += DC_NT_B) s_map[k] = class_map ? class_map[k] : k;
    if (feasible && tid < 64) {                                     // wave 0 walks from (F - 1, last) to frame 0
        int c = last, t = F - 1;
        while (true) {
            const uint8_t* __restrict__ col = Mv + (size_t)c * stride;
            int tp = 0, hi = t;                                     // tp: the frame of the advance into the last state; 0: none
            uint32_t m = 0;
            while (hi >= 1) {
                const int tt = hi - tid;
                m = tt >= 1 ? col[tt] : 0u;
                const unsigned long long bal = __ballot(m & 128u);
                if (bal) { tp = hi - (int)__builtin_ctzll(bal); break; }
                hi -= 64;
            }
            const int start = max(tp - (M - 1), 0);                 // the segment's first frame
            for (int tt = start + tid; tt <= t; tt += 64) s_fc[tt] = (uint8_t)c;
            if (start == 0) break;
            const int off = hi - start;                             // the lane that holds the byte at (start, c), if any
            const uint32_t mb = off < 64 ? (uint32_t)__shfl((int)m, off, 64) : (uint32_t)col[start];
            c = __builtin_amdgcn_readfirstlane(min((int)(mb & 127u), C - 1));
            t = start - 1;
        }
    }
    __syncthreads();
    int32_t* const out_f = frame_class + (size_t)b * max_frames;
    for (int t = tid; t < max_frames; t += DC_NT_B) out_f[t] = t < Fe ? (int)s_fc[t] : -1;
    // segments: the maximal runs of mapped labels that are not -1
    const int per = (Fe + DC_NT_B - 1) / DC_NT_B;
    const int t0 = min(tid * per, Fe), t1 = min(t0 + per, Fe);
    uint32_t cnt = 0;
    for (int t = t0; t < t1; ++t) {
        const int l = s_map[s_fc[t]];
        const int lp = t > 0 ? s_map[s_fc[t - 1]] : -2;
        const int ln = t + 1 < Fe ? s_map[s_fc[t + 1]] : -2;
        if (l != -1 && l != lp) cnt += 1u;
        if (l != -1 && l != ln) cnt += 1u << 16;
    }
    int sb = 0;
    s_scan[0][tid] = cnt;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < DC_NT_B; o <<= 1) {                         // inclusive scan, two buffers in turn
        const uint32_t v = s_scan[sb][tid] + (tid >= o ? s_scan[sb][tid - o] : 0u);
        sb ^= 1;
        s_scan[sb][tid] = v;
        __syncthreads();
    }
    const uint32_t incl = s_scan[sb][tid];
    const int ns = (int)(s_scan[sb][DC_NT_B - 1] & 0xffffu);
    int ks = (int)((incl - cnt) & 0xffffu), ke = (int)((incl - cnt) >> 16);
    int32_t* const o_lab = seg_label + (size_t)b * max_frames;
    int32_t* const o_st = seg_start + (size_t)b * max_frames;
    int32_t* const o_en = seg_end + (size_t)b * max_frames;
    float* const o_sc = seg_score + (size_t)b * max_frames;
    for (int t = t0; t < t1; ++t) {
        const int l = s_map[s_fc[t]];
        const int lp = t > 0 ? s_map[s_fc[t - 1]] : -2;
        const int ln = t + 1 < Fe ? s_map[s_fc[t + 1]] : -2;
        if (l != -1 && l != lp) { o_lab[ks] = l; o_st[ks] = t; s_st[ks] = (uint16_t)t; ++ks; }
        if (l != -1 && l != ln) { o_en[ke] = t + 1; s_en[ke] = (uint16_t)t; ++ke; }      // (LDS keeps the LAST frame: 16 bits)
    }
    for (int k = ns + tid; k < max_frames; k += DC_NT_B) {
        o_lab[k] = -1; o_st[k] = -1; o_en[k] = -1;
        o_sc[k] = __builtin_nanf("");
    }
    if (tid == 0) n_seg[b] = ns;
    __syncthreads();
    for (int k = tid; k < ns; k += DC_NT_B) {
        const int st = s_st[k], en = (int)s_en[k] + 1;
        double acc = 0.0;
        for (int t = st; t < en; ++t) acc += (double)E[(size_t)t * C + s_fc[t]];
        o_sc[k] = (float)(acc / (double)(en - st));
    }
}

}  // namespace

extern "C" {

size_t vc_decode_workspace_bytes(int32_t batch, int32_t max_frames, int32_t n_classes) {
    if (!dc_shape_ok(batch, max_frames, n_classes)) return 0;
    return dc_ws_bytes(batch, max_frames, n_classes);
}

int vc_decode_f32(const float* d_score, const int32_t* d_n_frames, const float* d_trans, const float* d_init, const float* d_final,
                  const int32_t* d_class_map, int32_t batch, int32_t max_frames, int32_t n_classes, int32_t min_dur,
                  int32_t* d_frame_class, int32_t* d_seg_label, int32_t* d_seg_start, int32_t* d_seg_end, int32_t* d_n_seg,
                  float* d_seg_score, float* d_total, void* d_workspace, size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_score && d_n_frames && d_trans && d_frame_class && d_seg_label && d_seg_start && d_seg_end && d_n_seg && d_seg_score &&
               d_total && d_workspace, "vc_decode_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_classes >= 1,
               "vc_decode_f32: bad shape (batch %d, max_frames %d, n_classes %d; need all >= 1)", batch, max_frames, n_classes);
    if (min_dur < 1 || min_dur > DC_MAX_DUR || !dc_shape_ok(batch, max_frames, n_classes))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_decode_f32: limits are batch <= 65535, max_frames <= %d, n_classes <= %d, min_dur in "
                             "[1, %d] and a workspace below 2 GiB; got batch %d, max_frames %d, n_classes %d, min_dur %d", DC_MAX_FRAMES,
                             DC_MAX_CLASSES, DC_MAX_DUR, batch, max_frames, n_classes, min_dur);
    VC_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 3) == 0, "vc_decode_f32: unaligned workspace");
    const size_t need = dc_ws_bytes(batch, max_frames, n_classes);
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_decode_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* fin = static_cast<int32_t*>(d_workspace);
    uint32_t* moves = reinterpret_cast<uint32_t*>(static_cast<char*>(d_workspace) + vc::align256((size_t)batch * sizeof(int32_t)));
    if (int rc = vc::allow_dynamic_lds<decode_forward_kernel<2>, decode_backtrack_kernel>(DC_FWD_LDS > DC_BT_LDS ? DC_FWD_LDS : DC_BT_LDS)) return rc;
    if (n_classes <= 64)
        hipLaunchKernelGGL(decode_forward_kernel<1>, dim3(batch), dim3(64), 0, st, d_score, d_n_frames, d_trans, d_init, d_final, max_frames,
                           n_classes, min_dur, d_total, fin, moves);
    else
        hipLaunchKernelGGL(decode_forward_kernel<2>, dim3(batch), dim3(128), (size_t)(n_classes * n_classes + 256) * sizeof(float), st, d_score,
                           d_n_frames, d_trans, d_init, d_final, max_frames, n_classes, min_dur, d_total, fin, moves);
    VC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(decode_backtrack_kernel, dim3(batch), dim3(DC_NT_B), (size_t)max_frames * 5, st, d_score, d_n_frames, d_class_map,
                       max_frames, n_classes, min_dur, fin, moves, d_frame_class, d_seg_label, d_seg_start, d_seg_end, d_n_seg, d_seg_score);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
