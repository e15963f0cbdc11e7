// Duration conversion on the device (include/vc_hip.h, "Duration"): a time map from a segment table, and the resampling
// of a spectrogram along it.
//
//   duration_map_kernel  segment table (start, end [, label] [, out_len]) + rates -> pos [B, Fw] (Q16 input frames per
//                        output frame), n_out, the segment table in output frames, flags.  Integer arithmetic only.
//   time_warp_kernel     x [B, F, C], pos, n_out -> y [B, Fw, C]: two source rows per output row, a + w * (b - a);
//                        optionally also the vocoder's magnitude of y (vc::power_db_to_amp, realse == 1)
//
// duration_map_kernel: one workgroup of 1,024 lanes per utterance.  Table entry k stands for two pieces, the gap before
// segment k and the segment itself (both empty for an absent entry); a last gap runs to the utterance's end.
//   1. The table goes through in tiles of 1,024 entries, lane t owning entry k0 + t.  The end of the last present segment
//      before it is an exclusive max scan (the running maximum of the present ends: for a sorted table the previous end,
//      for any other one the value that shows the overlap), the output offset an exclusive sum scan of the two pieces'
//      output lengths; carried from tile to tile in registers, the same in every lane: the running end, the running offset
//      and "a bad entry so far".  (offset, previous end) of every entry and of the last gap go to the workspace.  Output
//      lengths enter the offsets saturated at Fw + 1: an offset past Fw is never looked at, so 32 bits hold every sum.
//   2. The total decides the flags and n_out; every lane holds them.  The output table is one more pass over the entries.
//   3. Output frame u (lanes strided over [0, Fw)) finds the last entry whose offset is <= u by a binary search over the
//      workspace's offsets (an entry of no frames is never that one: its successor has the same offset), tells the gap
//      from the segment and divides once: pos = S * 2^16 + ((2j + 1) Li 2^16) / (2 Lo) - 2^15, clamped to the utterance.
// Every value read from the table is range-checked before it is used; nothing read from it forms an address.
//
// time_warp_kernel streams like the kernels of vc_convert.hip: no LDS, no atomics, every destination element written once;
// a destination slab [Fw * C] is a flat array, 16 bytes stored per lane when its length is a multiple of 4 floats; the two
// source rows are read as 16 bytes when C % 4 == 0 (a lane's four elements then lie in one row at an aligned address)
// and element by element otherwise (C = 201, 61).
#include "vc_common.h"

namespace {

constexpr int NT_M = 1024;              // lanes and tile of the map kernel
constexpr int NW_M = NT_M / 64;
constexpr int CT = 256;                 // lanes of the warp kernel
constexpr int MAX_SEG = 16384;
constexpr int MAX_FRAMES = 16384;
constexpr int Q_ONE = 65536;
constexpr int RATIO_MAX_Q = 8 * Q_ONE;
constexpr int FLAG_INVALID = 1, FLAG_SHORT = 2, FLAG_TRUNCATED = 4;

struct MapArgs {
    const int32_t* start;               // [B, K]
    const int32_t* end;
    const int32_t* n_seg;               // [B]
    const int32_t* label;               // [B, K] or NULL
    const int32_t* out_len;             // [B, K] or NULL
    const int32_t* ratio_q;             // [n_classes] or NULL
    const int32_t* n_frames;            // [B]
    int n_classes, gap_q, K, max_frames, min_frames, Fw;
    int32_t* pos;                       // [B, Fw]
    int32_t* n_out;                     // [B]
    int32_t* out_start;                 // [B, K]
    int32_t* out_end;
    int32_t* flags;                     // [B]
    int2* ws;                           // [B, K + 1] (output offset, previous end)
};

__device__ __forceinline__ long long scaled(int Li, int q) {
    return ((long long)Li * min(max(q, 0), RATIO_MAX_Q) + 32768) >> 16;
}

// Output length of the present segment k of Li frames, -1 when the table does not give one (a negative explicit length,
// a label outside the rate table).
__device__ __forceinline__ long long segment_out_len(const MapArgs& a, size_t row, int k, int Li) {
    if (a.out_len) {
        const int v = a.out_len[row + k];
        return v < 0 ? -1 : v;
    }
    if (!a.ratio_q) return Li;
    const int c = a.label ? a.label[row + k] : 0;
    if ((unsigned)c >= (unsigned)a.n_classes) return -1;
    return scaled(Li, a.ratio_q[c]);
}

__device__ __forceinline__ int piece_pos(int S, int Li, long long Lo, int j, int n) {
    const unsigned long long num = (unsigned long long)(2 * j + 1) * (unsigned long long)Li << 16;
    const long long p = ((long long)S << 16) + (long long)(num / (unsigned long long)(2 * Lo)) - 32768;
    return (int)min(max(p, 0ll), (long long)(n - 1) << 16);
}

__global__ void __launch_bounds__(NT_M)
duration_map_kernel(const MapArgs a) {
    __shared__ int wtot[NW_M];
    const int t = threadIdx.x, b = blockIdx.x;
    const int n = min(max(a.n_frames[b], 0), a.max_frames);
    const int n_seg = min(max(a.n_seg[b], 0), a.K);
    const size_t row = (size_t)b * a.K;
    int2* ws = a.ws + (size_t)b * (a.K + 1);
    const int cap = a.Fw + 1;
    // carried from tile to tile, the same in every lane
    int c_end = 0, c_off = 0, c_bad = 0;
    for (int k0 = 0; k0 < n_seg; k0 += NT_M) {
        const int k = k0 + t;
        const bool in = k < n_seg;
        const int s = in ? a.start[row + k] : -1, e = in ? a.end[row + k] : -1;
        const bool present = in && s >= 0 && e != s;
        bool ok = present && e > s && e <= n;
        int tot_end, tot_off;
        const int pe = max(vc::block_scan_excl<false, NW_M>(ok ? e : -1, wtot, tot_end), c_end);
        ok = ok && s >= pe;
        int w = 0;
        if (ok) {
            const long long lo_seg = segment_out_len(a, row, k, e - s);
            if (lo_seg < 0) ok = false;
            else w = (int)min(scaled(s - pe, a.gap_q), (long long)cap) + (int)min(lo_seg, (long long)cap);
        }
        const int off = c_off + vc::block_scan_excl<true, NW_M>(w, wtot, tot_off);
        if (in) ws[k] = make_int2(off, pe);
        c_bad |= __syncthreads_or(present && !ok);
        c_end = max(c_end, tot_end);
        c_off += tot_off;
    }
    const int tail = n - c_end;                                     // >= 0: every end that entered c_end is <= n
    const long long lo_tail = scaled(tail, a.gap_q);
    if (t == 0) ws[n_seg] = make_int2(c_off, c_end);
    const int total = c_off + (int)min(lo_tail, (long long)cap);
    int fl = 0;
    if (n > 0) fl = c_bad ? FLAG_INVALID : (total < a.min_frames ? FLAG_SHORT : 0);
    const bool identity = fl != 0;
    const int tot = n == 0 ? 0 : (identity ? n : total);
    if (tot > a.Fw) fl |= FLAG_TRUNCATED;
    const int n_out = min(tot, a.Fw);
    if (t == 0) { a.n_out[b] = n_out; a.flags[b] = fl; }
    __syncthreads();                                                // the workspace, before other lanes read it

    // the segment table in output frames
    for (int k = t; k < a.K; k += NT_M) {
        int os = -1, oe = -1;
        if (k < n_seg && n > 0 && !(fl & FLAG_INVALID)) {
            const int s = a.start[row + k], e = a.end[row + k];
            if (s >= 0 && e != s) {                                 // valid table: 0 <= s < e <= n
                if (identity) { os = s; oe = e; }
                else {
                    const int2 w = ws[k];
                    os = w.x + (int)min(scaled(s - w.y, a.gap_q), (long long)cap);
                    oe = os + (int)min(segment_out_len(a, row, k, e - s), (long long)cap);
                }
                os = min(os, n_out); oe = min(oe, n_out);
            }
        }
        a.out_start[row + k] = os;
        a.out_end[row + k] = oe;
    }

    // the map
    int32_t* pos = a.pos + (size_t)b * a.Fw;
    for (int u = t; u < a.Fw; u += NT_M) {
        int p = -1;
        if (u < n_out) {
            if (identity) p = u << 16;
            else {
                int lo = 0, hi = n_seg;                             // the last entry whose offset is <= u; ws[0].x == 0
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (ws[mid].x <= u) lo = mid; else hi = mid - 1;
                }
                const int2 w = ws[lo];
                const int jj = u - w.x;
                if (lo == n_seg) p = piece_pos(w.y, tail, lo_tail, jj, n);
                else {
                    const int s = a.start[row + lo], e = a.end[row + lo];
                    const long long lo_gap = scaled(s - w.y, a.gap_q);
                    if (jj < lo_gap) p = piece_pos(w.y, s - w.y, lo_gap, jj, n);
                    else p = piece_pos(s, e - s, segment_out_len(a, row, lo, e - s), jj - (int)lo_gap, n);
                }
            }
        }
        pos[u] = p;
    }
}

// The two source rows and the weight of output row t: i0 < 0 for a zero row.
struct WarpRow { int i0, i1; float w; };

__device__ __forceinline__ WarpRow warp_row(const int32_t* __restrict__ pos, int t, int n_out, int n, int nearest) {
    WarpRow r{-1, -1, 0.0f};
    if (t >= n_out || n <= 0) return r;
    const int p = min(max(pos[t], 0), (n - 1) << 16);
    if (nearest) {
        r.i0 = r.i1 = min((p + 32768) >> 16, n - 1);
    } else {
        r.i0 = p >> 16;
        r.i1 = min(r.i0 + 1, n - 1);
        r.w = (float)(p & 65535) * 1.52587890625e-5f;               // exact
    }
    return r;
}

// three separately rounded operations; w == 0 is the row itself whatever its neighbour holds.  (The pragma, not
// __fmul_rn / __fadd_rn: those are plain operators to this compiler, which contracts them into one fma.)
__device__ __forceinline__ float lerp_rn(float x0, float x1, float w) {
#pragma clang fp contract(off)
    const float d = x1 - x0;
    const float m = w * d;
    return x0 + m;
}

// grid (tiles of CT * V elements, B)
template <int V, bool ROWVEC>
__global__ void __launch_bounds__(CT)
time_warp_kernel(const float* __restrict__ src, const int32_t* __restrict__ pos_all, const int32_t* __restrict__ n_out_all,
                 const int32_t* __restrict__ n_frames, int F, int Fw, int C, int nearest, float inv_norm,
                 float* __restrict__ dst, float* __restrict__ amp) {
    const int b = blockIdx.y;
    const int slab = Fw * C;
    const int i0 = (blockIdx.x * CT + threadIdx.x) * V;
    if (i0 >= slab) return;
    const int n = min(max(n_frames ? n_frames[b] : F, 0), F);
    const int n_out = min(max(n_out_all[b], 0), Fw);
    const int32_t* __restrict__ pos = pos_all + (size_t)b * Fw;
    const float* __restrict__ x = src + (size_t)b * F * C;
    int t = i0 / C, c = i0 - t * C;
    float v[V], m[V];
    if (ROWVEC) {
        const WarpRow r = warp_row(pos, t, n_out, n, nearest);
        if (r.i0 >= 0) {
            const float4 p0 = *reinterpret_cast<const float4*>(x + (size_t)r.i0 * C + c);
            v[0] = p0.x; v[1] = p0.y; v[2] = p0.z; v[3] = p0.w;
            if (r.w != 0.0f) {
                const float4 p1 = *reinterpret_cast<const float4*>(x + (size_t)r.i1 * C + c);
                v[0] = lerp_rn(v[0], p1.x, r.w); v[1] = lerp_rn(v[1], p1.y, r.w);
                v[2] = lerp_rn(v[2], p1.z, r.w); v[3] = lerp_rn(v[3], p1.w, r.w);
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = (amp && r.i0 >= 0) ? vc::power_db_to_amp(v[k], inv_norm) : 0.0f;
    } else {
        WarpRow r = warp_row(pos, t, n_out, n, nearest);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = 0.0f;
            if (r.i0 >= 0) {
                v[k] = x[(size_t)r.i0 * C + c];
                if (r.w != 0.0f) v[k] = lerp_rn(v[k], x[(size_t)r.i1 * C + c], r.w);
            }
            m[k] = (amp && r.i0 >= 0) ? vc::power_db_to_amp(v[k], inv_norm) : 0.0f;
            if (++c == C) { c = 0; ++t; r = warp_row(pos, t, n_out, n, nearest); }     // (t == Fw >= n_out: a zero row, nothing read)
        }
    }
    float* o = dst + (size_t)b * slab + i0;
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        if (amp) *reinterpret_cast<float4*>(amp + (size_t)b * slab + i0) = make_float4(m[0], m[1], m[2], m[3]);
    } else {
        o[0] = v[0];
        if (amp) amp[(size_t)b * slab + i0] = m[0];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned tiles(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool map_shape_ok(int batch, int max_seg, int max_frames, int out_frames) {
    return batch >= 1 && batch <= 65535 && max_seg >= 1 && max_seg <= MAX_SEG && max_frames >= 1 && max_frames <= MAX_FRAMES &&
           out_frames >= 1 && out_frames <= MAX_FRAMES;
}

}  // namespace

extern "C" {

size_t vc_duration_map_workspace_bytes(int32_t batch, int32_t max_seg) {
    if (batch < 1 || batch > 65535 || max_seg < 1 || max_seg > MAX_SEG) return 0;
    return align256((size_t)batch * (max_seg + 1) * sizeof(int2));
}

int vc_duration_map(const int32_t* d_start, const int32_t* d_end, const int32_t* d_n_seg, const int32_t* d_label,
                    const int32_t* d_out_len, const int32_t* d_ratio_q, int32_t n_classes, int32_t gap_q,
                    const int32_t* d_n_frames, int32_t batch, int32_t max_seg, int32_t max_frames, int32_t min_frames,
                    int32_t out_frames, int32_t* d_pos, int32_t* d_n_out, int32_t* d_out_start, int32_t* d_out_end,
                    int32_t* d_flags, void* d_workspace, size_t workspace_bytes, void* stream) {
    VC_REQUIRE(d_start && d_end && d_n_seg && d_n_frames && d_pos && d_n_out && d_out_start && d_out_end && d_flags && d_workspace,
               "vc_duration_map: NULL argument");
    VC_REQUIRE(batch >= 1 && max_seg >= 1 && max_frames >= 1 && out_frames >= 1 && min_frames >= 0,
               "vc_duration_map: bad shape (batch %d, max_seg %d, max_frames %d, out_frames %d, min_frames %d)", batch, max_seg,
               max_frames, out_frames, min_frames);
    VC_REQUIRE(!(d_out_len && d_ratio_q), "vc_duration_map: explicit lengths and a rate table exclude each other");
    VC_REQUIRE(!d_label || d_ratio_q, "vc_duration_map: labels are for a rate table");
    VC_REQUIRE(!d_ratio_q || n_classes >= 1, "vc_duration_map: a rate table needs n_classes >= 1");
    VC_REQUIRE(!d_ratio_q || d_label || n_classes == 1, "vc_duration_map: without labels the rate table has one entry");
    if (!map_shape_ok(batch, max_seg, max_frames, out_frames) || gap_q < 0 || gap_q > RATIO_MAX_Q)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_duration_map: limits are batch <= 65535, max_seg, max_frames, out_frames <= %d "
                             "and gap_q in [0, %d]; got batch %d, max_seg %d, max_frames %d, out_frames %d, gap_q %d", MAX_FRAMES,
                             RATIO_MAX_Q, batch, max_seg, max_frames, out_frames, gap_q);
    if (workspace_bytes < vc_duration_map_workspace_bytes(batch, max_seg))
        return vc::set_error(VC_ERR_WORKSPACE, "vc_duration_map: workspace of %zu bytes, need %zu", workspace_bytes,
                             vc_duration_map_workspace_bytes(batch, max_seg));
    VC_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, "vc_duration_map: the workspace must be 8-byte aligned");
    MapArgs a;
    a.start = d_start; a.end = d_end; a.n_seg = d_n_seg; a.label = d_label; a.out_len = d_out_len; a.ratio_q = d_ratio_q;
    a.n_frames = d_n_frames; a.n_classes = n_classes; a.gap_q = gap_q; a.K = max_seg; a.max_frames = max_frames;
    a.min_frames = min_frames; a.Fw = out_frames; a.pos = d_pos; a.n_out = d_n_out; a.out_start = d_out_start;
    a.out_end = d_out_end; a.flags = d_flags; a.ws = static_cast<int2*>(d_workspace);
    hipLaunchKernelGGL(duration_map_kernel, dim3(batch), dim3(NT_M), 0, static_cast<hipStream_t>(stream), a);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_time_warp(const float* d_src, const int32_t* d_pos, const int32_t* d_n_out, const int32_t* d_n_frames, int32_t batch,
                 int32_t max_frames, int32_t out_frames, int32_t C, int32_t mode, float* d_dst, float* d_amp,
                 float P_dB_norm_factor, void* stream) {
    VC_REQUIRE(d_src && d_pos && d_n_out && d_dst, "vc_time_warp: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && out_frames >= 1 && C >= 1, "vc_time_warp: bad shape (batch %d, max_frames %d, "
               "out_frames %d, C %d)", batch, max_frames, out_frames, C);
    VC_REQUIRE(mode == VC_WARP_LINEAR || mode == VC_WARP_NEAREST, "vc_time_warp: mode must be VC_WARP_LINEAR or VC_WARP_NEAREST");
    VC_REQUIRE(!d_amp || P_dB_norm_factor != 0.0f, "vc_time_warp: P_dB_norm_factor is 0");
    if (batch > 65535 || max_frames > MAX_FRAMES || out_frames > MAX_FRAMES || (long long)out_frames * C >= (1ll << 30) ||
        (long long)max_frames * C >= (1ll << 30))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_time_warp: limits are batch <= 65535, max_frames, out_frames <= %d and "
                             "frames * C < 2^30; got batch %d, max_frames %d, out_frames %d, C %d", MAX_FRAMES, batch, max_frames,
                             out_frames, C);
    const float inv_norm = d_amp ? 1.0f / P_dB_norm_factor : 0.0f;
    const long long slab = (long long)out_frames * C;
    const int nearest = mode == VC_WARP_NEAREST;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (slab % 4) == 0 && aligned16(d_dst) && (!d_amp || aligned16(d_amp));
    if (vec && (C % 4) == 0 && aligned16(d_src))
        hipLaunchKernelGGL((time_warp_kernel<4, true>), dim3(tiles(slab, CT * 4), batch), dim3(CT), 0, st, d_src, d_pos, d_n_out,
                           d_n_frames, max_frames, out_frames, C, nearest, inv_norm, d_dst, d_amp);
    else if (vec)
        hipLaunchKernelGGL((time_warp_kernel<4, false>), dim3(tiles(slab, CT * 4), batch), dim3(CT), 0, st, d_src, d_pos, d_n_out,
                           d_n_frames, max_frames, out_frames, C, nearest, inv_norm, d_dst, d_amp);
    else
        hipLaunchKernelGGL((time_warp_kernel<1, false>), dim3(tiles(slab, CT), batch), dim3(CT), 0, st, d_src, d_pos, d_n_out,
                           d_n_frames, max_frames, out_frames, C, nearest, inv_norm, d_dst, d_amp);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
