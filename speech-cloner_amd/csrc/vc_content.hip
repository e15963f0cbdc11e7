// Content preservation on the device (include/vc_hip.h, "Content"): the frame-level agreement of two phoneme
// posteriorgrams along a set of cells, the phoneme sequence of a posteriorgram, and the edit distance of two sequences
// with the counts behind it.
//
//     js(i, j) = 0.5 * sum_c (p log2(p / m) + q log2(q / m)),  p = a[i, c], q = b[j, c], m = (p + q) / 2     (bits)
//     l[f]     = map[argmax_c ppg[f, c]];  runs of equal l;  runs shorter than min_run removed;  equal neighbours merged;
//                segments labelled -1 removed
//     E(i, j)  = min(E(i-1, j-1) + [a_i != b_j], E(i-1, j) + 1, E(i, j-1) + 1), ties diagonal, up, left; every cell
//                carries (n_match, n_sub, n_del, n_ins) from its chosen predecessor
//
// ppg_metrics_kernel: one workgroup of sixteen waves per pair, one wave per cell (wave w takes cells w, w + 16, ...).  Lane l
// holds classes l, l + 64, l + 128, l + 192 of both rows: consecutive lanes read consecutive words.  A lane adds its
// classes' terms in float64, c ascending; the 64 partial sums are added in a butterfly (lane l adds lane l ^ 32, then
// l ^ 16, ... l ^ 1) and so is the arg-max (larger value, lower index on equality).  A wave adds its cells' js in cell
// order; the sixteen waves' sums are added in the order 0 .. 15.  No LDS beyond those partial sums, one barrier.
//
// phn_segments_kernel: one workgroup of 1,024 lanes per utterance, tiles of 1,024 positions, position f = 0 .. F (F is a
// virtual frame whose label equals no other: it closes the last run).  A tile's labels come from one wave per frame (the
// butterfly arg-max above) and go to LDS; then lane t owns position t0 + t.  A position that starts a run completes
// the run before it; that run's start is the last start before it (exclusive max scan), the survivor before a
// survivor is the last completed run of at least min_run frames (exclusive max scan), and a survivor whose label
// differs from that one's heads a segment; the position of a head in the output is the count of heads before it whose
// label is not -1 (exclusive sum scan).  A head writes its label and start and the end of the segment before it; the
// last segment's end is written after the last tile.  Scans: Kogge-Stone inside a wave by shuffles, the sixteen wave
// totals through LDS -- two barriers a scan, three scans a tile.  Carried from tile to tile, in registers, the same in
// every lane: the last label, the last start, the last survivor (label, end) and the count.  No workspace.
//
// edit_distance_kernel: one workgroup of ONE wave per pair, R = 4 consecutive symbols of A per lane: a pass covers
// 64 * R = 256 rows.  Lane t works on column j = s - t at step s (an anti-diagonal of the lane grid); what it needs from
// above -- the cell of lane t - 1's last row at column j -- was produced one step earlier and comes by a shuffle, and so
// does b[j], handed from lane to lane; the value that came one step earlier is the diagonal.  No LDS, no barrier inside a
// pass.  Every 64 steps the lanes read the next 64 symbols of B (and, after the first pass, the next 64 cells of the
// row above the pass) with one coalesced load each; lane 0 takes its column's out of them by a shuffle.  The last row
// of a full pass goes through two rows of cells per pair in the workspace (16 bytes a cell), written by lane 63.
//
// Every result is a function of its own pair or utterance alone: fixed geometry, fixed orders, no atomics.
#include <cmath>
#include "vc_device.h"

namespace {

constexpr int MAX_CLASSES = 256;
constexpr int MAX_CELLS = 1 << 30;
constexpr int NT_P = 1024;              // lanes of the metrics kernel: sixteen waves, a cell each
constexpr int NT_S = 1024;              // lanes and tile of the segment kernel
constexpr int NW_S = NT_S / 64;
constexpr int ED_R = 4;                 // symbols of A per lane
constexpr int ED_ROWS = 64 * ED_R;      // rows per pass
constexpr int ED_MAX = 16384;
constexpr int NO_LABEL = -0x7fffffff - 1;       // the label of the virtual frame F and of "nothing before frame 0"

// arg-max of one row of n_classes floats over a wave, lowest index on equality; the same value in every lane
__device__ inline int wave_argmax(const float* __restrict__ row, int n_classes, int lane) {
    float v = -__builtin_inff();
    int idx = 0x7fffffff;
    for (int c = lane; c < n_classes; c += 64) {
        const float x = row[c];
        if (x > v || idx == 0x7fffffff) { v = x; idx = c; }
    }
    return vc::wave_argmax_low(v, idx).idx;
}

__device__ inline double js_term(double p, double m) { return p > 0.0 ? p * log2(p / m) : 0.0; }

// counts [batch, 2]: n_cells, n_agree.  values [batch, 2]: frame_agreement, js_mean.
__global__ void __launch_bounds__(NT_P)
ppg_metrics_kernel(const float* __restrict__ ppg_a, const float* __restrict__ ppg_b, const int32_t* __restrict__ len_a,
                   const int32_t* __restrict__ len_b, int max_a, int max_b, int n_classes, const int32_t* __restrict__ path,
                   const int32_t* __restrict__ path_len, int max_path, const int32_t* __restrict__ class_map,
                   int32_t* __restrict__ counts, float* __restrict__ values) {
    __shared__ double w_js[NT_P / 64];
    __shared__ int w_cells[NT_P / 64], w_agree[NT_P / 64];
    const int p = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int la = min(max(len_a[p], 1), max_a);
    const int lb = min(max(len_b[p], 1), max_b);
    const float* __restrict__ A = ppg_a + (size_t)p * max_a * n_classes;
    const float* __restrict__ B = ppg_b + (size_t)p * max_b * n_classes;
    const int32_t* __restrict__ P = path ? path + (size_t)p * max_path * 2 : nullptr;
    const int n = path ? min(max(path_len[p], 0), max_path) : min(la, lb);
    double js_sum = 0.0;
    int cells = 0, agree = 0;
    for (int k = wave; k < n; k += NT_P / 64) {                     // uniform over the wave
        const int i = P ? P[2 * k] : k, j = P ? P[2 * k + 1] : k;
        if (i < 0 || i >= la || j < 0 || j >= lb) continue;
        const float* __restrict__ ra = A + (size_t)i * n_classes;
        const float* __restrict__ rb = B + (size_t)j * n_classes;
        double acc = 0.0;
        float va = -__builtin_inff(), vb = -__builtin_inff();
        int ia = 0x7fffffff, ib = 0x7fffffff;
        for (int c = lane; c < n_classes; c += 64) {
            const float fa = ra[c], fb = rb[c];
            if (fa > va || ia == 0x7fffffff) { va = fa; ia = c; }
            if (fb > vb || ib == 0x7fffffff) { vb = fb; ib = c; }
            const double pa = (double)fa, pb = (double)fb, m = 0.5 * (pa + pb);
            acc += js_term(pa, m) + js_term(pb, m);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
        ia = vc::wave_argmax_low(va, ia).idx;
        ib = vc::wave_argmax_low(vb, ib).idx;
        js_sum += 0.5 * acc;
        ++cells;
        if (class_map) { ia = class_map[ia]; ib = class_map[ib]; }
        if (ia == ib) ++agree;
    }
    if (lane == 0) { w_js[wave] = js_sum; w_cells[wave] = cells; w_agree[wave] = agree; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = w_js[0];
        int nc = w_cells[0], na = w_agree[0];
        for (int w = 1; w < NT_P / 64; ++w) { s += w_js[w]; nc += w_cells[w]; na += w_agree[w]; }
        const float nan = __builtin_nanf("");
        counts[2 * p] = nc;
        counts[2 * p + 1] = na;
        values[2 * p] = nc > 0 ? (float)((double)na / (double)nc) : nan;
        values[2 * p + 1] = nc > 0 ? (float)(s / (double)nc) : nan;
    }
}

__global__ void __launch_bounds__(NT_S)
phn_segments_kernel(const float* __restrict__ ppg, const int32_t* __restrict__ n_frames, int max_frames, int n_classes,
                    int min_run, const int32_t* __restrict__ class_map, int32_t* __restrict__ labels,
                    int32_t* __restrict__ start, int32_t* __restrict__ end, int32_t* __restrict__ n_seg) {
    __shared__ int lab[NT_S];
    __shared__ int wtot[NW_S];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x;
    const int F = min(max(n_frames[b], 0), max_frames);
    const float* __restrict__ X = ppg + (size_t)b * max_frames * n_classes;
    int32_t* out_l = labels + (size_t)b * max_frames;
    int32_t* out_s = start + (size_t)b * max_frames;
    int32_t* out_e = end + (size_t)b * max_frames;
    // carried from tile to tile, the same in every lane
    int c_lab = NO_LABEL;               // label of the position before the tile
    int c_start = -1;                   // the last run start so far
    bool c_have = false;                // a survivor so far, its label and end
    int c_slab = 0, c_send = 0;
    int c_count = 0;                    // segments written so far
    for (int t0 = 0; t0 <= F; t0 += NT_S) {                         // positions 0 .. F
        const int n_here = min(NT_S, F + 1 - t0);
        __syncthreads();                                            // the previous tile's reads of lab
        for (int k = wave; k < n_here; k += NW_S) {                 // uniform over the wave
            const int f = t0 + k;
            int l = NO_LABEL;
            if (f < F) {
                l = wave_argmax(X + (size_t)f * n_classes, n_classes, lane);
                if (class_map) l = class_map[l];
            }
            if (lane == 0) lab[k] = l;
        }
        __syncthreads();
        const int f = t0 + t;
        const bool in = t < n_here;
        const int mine = in ? lab[t] : NO_LABEL;
        const int before = t > 0 ? lab[min(t, n_here) - 1] : c_lab;        // (lanes beyond the tile read a valid slot)
        const bool is_start = in && (f == 0 || mine != before);
        int tot_start, tot_surv, tot_emit;
        // the run [rs, f) with label `before` completes at a start f > 0
        const int rs = max(vc::block_scan_excl<false, NW_S>(is_start ? f : -1, wtot, tot_start), c_start);
        const bool surv = is_start && f > 0 && f - rs >= min_run;
        const int tp = vc::block_scan_excl<false, NW_S>(surv ? t : -1, wtot, tot_surv);         // the survivor before, as a lane of this tile
        bool have = c_have;
        int plab = c_slab, pend = c_send;
        if (tp >= 0) { have = true; plab = tp > 0 ? lab[tp - 1] : c_lab; pend = t0 + tp; }
        const bool head = surv && (!have || plab != before);
        const bool emit = head && before != -1;
        const int k = c_count + vc::block_scan_excl<true, NW_S>(emit ? 1 : 0, wtot, tot_emit);
        if (emit) { out_l[k] = before; out_s[k] = rs; }
        if (head && have && plab != -1) out_e[k - 1] = pend;
        // the carry
        if (tot_surv >= 0) { c_have = true; c_slab = tot_surv > 0 ? lab[tot_surv - 1] : c_lab; c_send = t0 + tot_surv; }
        c_lab = lab[n_here - 1];
        c_start = max(c_start, tot_start);
        c_count += tot_emit;
    }
    if (t == 0) {
        if (c_have && c_slab != -1) out_e[c_count - 1] = c_send;
        n_seg[b] = c_count;
    }
    for (int k = c_count + t; k < max_frames; k += NT_S) { out_l[k] = -1; out_s[k] = -1; out_e[k] = -1; }
}

struct ECell {                          // E and three of the four counts of one cell; n_ins = E - n_sub - n_del
    int32_t E, m, s, d;
};

__device__ inline ECell shfl_up_cell(const ECell& c) {
    return ECell{__shfl_up(c.E, 1, 64), __shfl_up(c.m, 1, 64), __shfl_up(c.s, 1, 64), __shfl_up(c.d, 1, 64)};
}
__device__ inline ECell shfl_cell(const ECell& c, int src) {
    return ECell{__shfl(c.E, src, 64), __shfl(c.m, src, 64), __shfl(c.s, src, 64), __shfl(c.d, src, 64)};
}

inline bool ed_shape_ok(int batch, int max_a, int max_b) {
    return batch >= 1 && batch <= 65535 && max_a >= 1 && max_a <= ED_MAX && max_b >= 1 && max_b <= ED_MAX;
}

// counts [batch, 5]: dist, n_match, n_sub, n_del, n_ins.  bound [batch][2][max_b] cells.
__global__ void __launch_bounds__(64)
edit_distance_kernel(const int32_t* __restrict__ seq_a, const int32_t* __restrict__ seq_b, const int32_t* __restrict__ n_a,
                     const int32_t* __restrict__ n_b, int max_a, int max_b, int32_t* __restrict__ counts,
                     float* __restrict__ per, ECell* bound) {
    const int p = blockIdx.x;
    const int t = threadIdx.x;
    const int Na = min(max(n_a[p], 0), max_a);
    const int Nb = min(max(n_b[p], 0), max_b);
    const int32_t* __restrict__ A = seq_a + (size_t)p * max_a;
    const int32_t* __restrict__ B = seq_b + (size_t)p * max_b;
    ECell* bnd = bound + (size_t)p * 2 * max_b;
    if (Na == 0 || Nb == 0) {                                       // all insertions, or all deletions (uniform)
        if (t == 0) {
            counts[5 * p] = Na + Nb;
            counts[5 * p + 1] = 0;
            counts[5 * p + 2] = 0;
            counts[5 * p + 3] = Na;
            counts[5 * p + 4] = Nb;
            per[p] = Na > 0 ? 1.0f : __builtin_nanf("");
        }
        return;
    }
    const int n_pass = (Na + ED_ROWS - 1) / ED_ROWS;
    for (int ps = 0; ps < n_pass; ++ps) {
        const int i0 = ps * ED_ROWS + t * ED_R;                     // this lane's first symbol of A
        const int rows_here = min(ED_ROWS, Na - ps * ED_ROWS);
        const int t_last = (rows_here - 1) / ED_R;
        const bool last_pass = ps == n_pass - 1;
        const ECell* bin = bnd + (size_t)(ps & 1) * max_b;          // written by pass ps - 1
        ECell* bout = bnd + (size_t)((ps + 1) & 1) * max_b;
        int32_t a[ED_R];
        ECell left[ED_R];                                           // column j - 1 of this lane's rows; column "-1" is E(i, 0) = i
#pragma unroll
        for (int r = 0; r < ED_R; ++r) {
            a[r] = i0 + r < Na ? A[i0 + r] : 0;
            left[r] = ECell{i0 + r + 1, 0, 0, i0 + r + 1};
        }
        ECell diag{i0, 0, 0, i0};                                   // the row above this lane's first, one column back
        ECell out{0, 0, 0, 0};                                      // this lane's last row at its column of the step before
        ECell top{0, 0, 0, 0};                                      // 64 cells of the row above the pass, one per lane
        int32_t bsym = 0, bchunk = 0;
        const int n_steps = Nb + t_last;
        __syncthreads();                                            // the previous pass's stores to bin
        for (int s = 0; s < n_steps; ++s) {
            if ((s & 63) == 0) {                                    // the next 64 columns
                const int j = s + t;
                bchunk = j < Nb ? B[j] : 0;
                if (ps > 0 && j < Nb) top = bin[j];
            }
            // every lane takes part in the shuffles; what an idle lane hands on is never used
            const ECell from_up = shfl_up_cell(out);
            const ECell from_top = shfl_cell(top, s & 63);
            const int32_t b_up = __shfl_up(bsym, 1, 64);
            const int32_t b_top = __shfl(bchunk, s & 63, 64);
            const int j = s - t;
            bsym = t == 0 ? b_top : b_up;
            const bool active = t <= t_last && j >= 0 && j < Nb;
            if (active) {
            const ECell up_in = t > 0 ? from_up : (ps > 0 ? from_top : ECell{j + 1, 0, 0, 0});
            ECell dg = diag, up = up_in;
#pragma unroll
            for (int r = 0; r < ED_R; ++r) {
                const bool sub = a[r] != bsym;
                ECell n{dg.E + (sub ? 1 : 0), dg.m + (sub ? 0 : 1), dg.s + (sub ? 1 : 0), dg.d};        // ties: diagonal, up, left
                if (up.E + 1 < n.E) n = ECell{up.E + 1, up.m, up.s, up.d + 1};
                if (left[r].E + 1 < n.E) n = ECell{left[r].E + 1, left[r].m, left[r].s, left[r].d};
                dg = left[r];                                       // (i, j-1) is the diagonal of row i + 1
                up = n;
                left[r] = n;
                if (last_pass && j == Nb - 1 && i0 + r == Na - 1) {
                    counts[5 * p] = n.E;
                    counts[5 * p + 1] = n.m;
                    counts[5 * p + 2] = n.s;
                    counts[5 * p + 3] = n.d;
                    counts[5 * p + 4] = n.E - n.s - n.d;
                    per[p] = (float)n.E / (float)Na;
                }
            }
            diag = up_in;
            out = up;
            if (!last_pass && t == 63) bout[j] = out;               // (only a full pass is followed by another)
            }
        }
    }
}

}  // namespace

extern "C" {

int vc_ppg_metrics_f32(const float* d_ppg_a, const float* d_ppg_b, const int32_t* d_len_a, const int32_t* d_len_b, int32_t batch,
                       int32_t max_a, int32_t max_b, int32_t n_classes, const int32_t* d_path, const int32_t* d_path_len,
                       int32_t max_path, const int32_t* d_class_map, int32_t* d_counts, float* d_values, void* stream) {
    VC_REQUIRE(d_ppg_a && d_ppg_b && d_len_a && d_len_b && d_counts && d_values, "vc_ppg_metrics_f32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_a >= 1 && max_b >= 1 && n_classes >= 1,
               "vc_ppg_metrics_f32: bad shape (batch %d, max_a %d, max_b %d, n_classes %d)", batch, max_a, max_b, n_classes);
    VC_REQUIRE((d_path == nullptr) == (d_path_len == nullptr) && (d_path ? max_path >= 1 : max_path == 0),
               "vc_ppg_metrics_f32: pass d_path, d_path_len and max_path >= 1 together, or NULL, NULL and 0 (max_path %d)", max_path);
    if (batch > 65535 || max_a > MAX_CELLS || max_b > MAX_CELLS || max_path > MAX_CELLS || n_classes > MAX_CLASSES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_ppg_metrics_f32: limits are batch <= 65535, max_a, max_b, max_path <= %d and "
                             "n_classes <= %d; got batch %d, max_a %d, max_b %d, max_path %d, n_classes %d", MAX_CELLS, MAX_CLASSES,
                             batch, max_a, max_b, max_path, n_classes);
    hipLaunchKernelGGL(ppg_metrics_kernel, dim3(batch), dim3(NT_P), 0, static_cast<hipStream_t>(stream), d_ppg_a, d_ppg_b, d_len_a,
                       d_len_b, max_a, max_b, n_classes, d_path, d_path_len, max_path, d_class_map, d_counts, d_values);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_phn_segments_tile(void) { return NT_S; }

int vc_phn_segments(const float* d_ppg, const int32_t* d_n_frames, int32_t batch, int32_t max_frames, int32_t n_classes,
                    int32_t min_run, const int32_t* d_class_map, int32_t* d_labels, int32_t* d_start, int32_t* d_end,
                    int32_t* d_n_seg, void* stream) {
    VC_REQUIRE(d_ppg && d_n_frames && d_labels && d_start && d_end && d_n_seg, "vc_phn_segments: NULL argument");
    VC_REQUIRE(batch >= 1 && max_frames >= 1 && n_classes >= 1 && min_run >= 1,
               "vc_phn_segments: bad shape (batch %d, max_frames %d, n_classes %d, min_run %d; need all >= 1)", batch, max_frames,
               n_classes, min_run);
    if (batch > 65535 || max_frames > MAX_CELLS || n_classes > MAX_CLASSES)
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_phn_segments: limits are batch <= 65535, max_frames <= %d and n_classes <= %d; got "
                             "batch %d, max_frames %d, n_classes %d", MAX_CELLS, MAX_CLASSES, batch, max_frames, n_classes);
    hipLaunchKernelGGL(phn_segments_kernel, dim3(batch), dim3(NT_S), 0, static_cast<hipStream_t>(stream), d_ppg, d_n_frames, max_frames,
                       n_classes, min_run, d_class_map, d_labels, d_start, d_end, d_n_seg);
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

int vc_edit_distance_rows(void) { return ED_ROWS; }

size_t vc_edit_distance_workspace_bytes(int32_t batch, int32_t max_a, int32_t max_b) {
    if (!ed_shape_ok(batch, max_a, max_b)) return 0;
    return vc::align256((size_t)batch * 2 * max_b * sizeof(ECell));
}

int vc_edit_distance_i32(const int32_t* d_seq_a, const int32_t* d_seq_b, const int32_t* d_n_a, const int32_t* d_n_b, int32_t batch,
                         int32_t max_a, int32_t max_b, int32_t* d_counts, float* d_per, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
    VC_REQUIRE(d_seq_a && d_seq_b && d_n_a && d_n_b && d_counts && d_per && d_workspace, "vc_edit_distance_i32: NULL argument");
    VC_REQUIRE(batch >= 1 && max_a >= 1 && max_b >= 1, "vc_edit_distance_i32: bad shape (batch %d, max_a %d, max_b %d)", batch, max_a,
               max_b);
    if (!ed_shape_ok(batch, max_a, max_b))
        return vc::set_error(VC_ERR_UNSUPPORTED, "vc_edit_distance_i32: limits are batch <= 65535 and max_a, max_b <= %d; got batch %d, "
                             "max_a %d, max_b %d", ED_MAX, batch, max_a, max_b);
    VC_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 15) == 0, "vc_edit_distance_i32: unaligned workspace");
    const size_t need = vc_edit_distance_workspace_bytes(batch, max_a, max_b);
    if (workspace_bytes < need)
        return vc::set_error(VC_ERR_WORKSPACE, "vc_edit_distance_i32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipLaunchKernelGGL(edit_distance_kernel, dim3(batch), dim3(64), 0, static_cast<hipStream_t>(stream), d_seq_a, d_seq_b, d_n_a, d_n_b,
                       max_a, max_b, d_counts, d_per, static_cast<ECell*>(d_workspace));
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

}  // extern "C"
