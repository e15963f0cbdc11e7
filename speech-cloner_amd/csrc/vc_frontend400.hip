// Signal front-end, shipped configuration (n_fft = 400, hop = 80, 80 mels, 40 cepstra): every output byte written
// exactly once (/root/reference/audio_lib.py:89-244), in one launch or in two.
//
// Both forms are built from ONE definition of each piece of arithmetic (the helpers below: the gather and the power
// rows of the tile transform, the two reductions, the utterance's constants, the output tail): the utterance's minimum
// maps to exactly 0, frame 0's own coefficient cancels to 0 and the no-wait path reproduces the published records
// because every value goes through the same function, whichever kernel calls it.  The kernels keep what differs --
// tiling, hand-off, what is kept where -- and, for a measured reason given in fe400_kernel, the text of the two DFT stages.
//
//   one launch   fe400_fused_kernel   (the default) every frame transformed once: a block transforms its 16 frames
//                                 (14 outputs + one halo frame each side), publishes its tile record, waits for the
//                                 records of its own utterance and finishes from LDS (see ONE-LAUNCH FORM below).
//                                 Reads 320 B/frame, writes 1,444 B/frame.
//   two launches (option fe_fused = 0, the throughput loop, utterances too long for vc_fe400_fused_ok):
//   pass 1  fe400_kernel<true>    16 frames per block: gather + reflect + pre-emphasis -> windowed 400-point real
//                                 DFT (25 x 16 split, fe_dft400.h) -> |.|^2 -> sparse Slaney mel; keeps ONLY the
//                                 tile's max / min of the power and of the mel power (linear: the dB maps are
//                                 monotone), sum|x| of its own samples, and frame 0's mel row.  Reads 320 B/frame,
//                                 writes 32 B per tile.
//   pass 2  fe400_kernel<false>   16 frames per block (14 output frames + one halo frame each side for the deltas):
//                                 the same transform again, then -- with the utterance's extremes known --
//                                 power_to_db + top_db clip + min shift + scale + clip -> P_dB, amplitude_to_db of
//                                 the mel POWER (the reference's quirk, audio_lib.py:172) -> M_dB, DCT-II (using
//                                 D[i][79-j] = (-1)^i D[i][j]: 40 instead of 80 products per coefficient), frame-0
//                                 shift, scale, delta, clip -> MFCC.  Reads 320 B/frame again (L2 / Infinity Cache
//                                 hits), writes 1,444 B/frame once.
// HBM traffic of the two launches: 2 x 320 + 1,444 = 2,084 B/frame against 1,764 algorithmic (1.18x); the three-launch
// form in vc_frontend.hip (kept for every other configuration) moves the raw dB tiles through HBM twice (2.4x).
// Recomputing the transform is the cheaper side of that trade: the kernels are issue- and latency-bound, not
// byte-bound, and the transform is ~40 % of a pass's instructions.
#include <hip/hip_runtime.h>
#include "vc_device.h"
#include "fe_dft400.h"
#include "vc_frontend400.h"

using vc::f32x4;

namespace {

constexpr int NT = 256;
constexpr int G = 16;                 // frames transformed per block
constexpr int GO = 14;                // output frames per block in pass 2
constexpr int HOP = 80, NFFT = 400, HALF = 200, NB = 201, NM = 80, NC = 40, NH = 40;
constexpr int WSPAN = HOP * 3 + NFFT;               // 640 samples under a wave's 4 frames
constexpr int RP = 20;                              // row pitch (floats): 16 + 4 pad -> ds_read_b128 of 16 consecutive rows
                                                    // conflict-free (5 r mod 16 is a permutation), every address an immediate
constexpr int WROWS = 52;                           // (frame, k1) rows of one wave: 4 frames x 13
constexpr int RE_W = WROWS * RP;                    // 1040 floats of real parts per wave
constexpr int IM_W = 48 * RP;                       // 960 floats of imaginary parts per wave (k1 = 0 is real: not stored)
constexpr int PP = RE_W / 4;                        // 260: pitch of a power-tile row (4 rows per wave region, 59 floats of slack each)
constexpr float NEG_INF = -3.402823466e38f, POS_INF = 3.402823466e38f;
constexpr float DB10 = 3.0102999566398120f;         // 10 log10(x) = DB10 * log2(x)

// LDS carve (floats): A_re [4 waves][52 rows] | A_im [4 waves][48 rows] | scalars.
// Everything up to the power tile is WAVE-LOCAL: a wave loads the 640 samples under its own 4 frames (into its own
// imaginary-row region, which it overwrites only after reading them: LDS operations of one wave execute in order), runs
// the 25-point stage on them, reads its own 52 rows back for the 16-point stage and writes its 4 power rows over its own
// real-row region.  No workgroup barrier before "power tile complete", so the four waves of a block -- and the blocks of
// a CU -- drift apart and one wave's load latency runs under another's arithmetic.  (Measured alternatives, all slower
// or equal: samples straight from global memory in the 25-point stage, 6-12 % slower (50 loads per thread against 14);
// a fifth block per CU by XOR-swizzled 16-float rows, no change: resident blocks are not the limit.)
constexpr int O_ARE = 0, O_AIM = 4 * RE_W, O_SC = O_AIM + 4 * IM_W, LDS_FLOATS = O_SC + 48;      // sc: [0, 9) constants, [16, 36) wave partials, [40] flag
// after the transform the imaginary rows are free: the output tail's tiles alias them
constexpr int O_MF = O_AIM;                          // [G][40]  scaled cepstra
constexpr int O_SD = O_AIM + G * NC;                 // [G][80]  j < 40: m[j] + m[79-j], j >= 40: m[j-40] - m[119-j]
constexpr int O_MC = O_AIM + G * NC + G * NM;        // [G][80]  clipped mel dB (one-launch form: the mel POWER until the constants are known)
static_assert(WSPAN <= IM_W, "a wave's samples alias its imaginary rows");
static_assert(PP >= NB + 14, "a power row plus the mel loop's over-read fit the row pitch");
static_assert(G * NC + 2 * G * NM <= 4 * IM_W, "cepstra + sum/difference + mel dB tiles alias the imaginary rows");
static_assert(4 * LDS_FLOATS * 4 <= 160 * 1024, "four blocks per CU");

__device__ __forceinline__ int utt_len(const Fe400Args& a, int b) {
    const int L = a.lens ? a.lens[b] : a.max_samples;
    return min(max(L, 1), a.max_samples);
}

// amplitude_to_db applied to the mel POWER (audio_lib.py:172: 10 log10(max(1e-10, v^2)) = 20 log10(max(1e-5, v))), the
// amplitude-normalisation offset, and the top_db floor.  One function: frame 0's reference value and the tile's own
// values must round identically.  (The amin clamp -100 dB is below every floor: floor >= -100.)
__device__ __forceinline__ float mel_db_clipped(float v, float offm, float mfloor) {
    return fmaxf(fmaf(2.0f * DB10, __log2f(fmaxf(v, 1e-18f)), offm), mfloor);
}

// power_to_db (audio_lib.py:157: 10 log10(max(1e-10, P)), then the top_db floor) with the amplitude-normalisation offset;
// the amin clamp sits 200 dB under the 1e-30 used here once the offset is added back, i.e. below every floor >= -100.
__device__ __forceinline__ float pow_db_clipped(float v, float offp, float pfloor) {
    return fmaxf(fmaf(DB10, __log2f(fmaxf(v, 1e-30f)), offp), pfloor);
}

// One filter of the sparse mel matrix on one frame: 14 reads issued together (reads past the filter's own count meet
// zero weights; past the tile's last row they meet the zero pad), then one FMA chain.  A per-term `if (j < count)`
// here serialised every LDS round trip behind a branch: 10,280 of a block's 20,810 cycles.
__device__ __forceinline__ float mel_dot(const float* p, const float (&w)[14]) {
    float v[14];
#pragma unroll
    for (int j = 0; j < 14; ++j) v[j] = p[j];
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < 14; ++j) acc = fmaf(w[j], v[j], acc);
    return acc;
}

// Loads and stores that bypass this CU's L1 (sc1): the one-launch form's hand-off (see ONE-LAUNCH FORM below).
__device__ __forceinline__ float ld_sc1(const float* p) {
    typedef __attribute__((address_space(1))) unsigned gu32;
    return __uint_as_float(__hip_atomic_load((gu32*)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_sc1(float* p, float v) {
    typedef __attribute__((address_space(1))) unsigned gu32;
    __hip_atomic_store((gu32*)(uintptr_t)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ============================================================================================================
// THE TILE TRANSFORM: 16 frames from f0 on -> the power tile (row g at smem + O_ARE + g * PP), in the phases its
// callers need (the feature pass computes the utterance's constants between load_samples and store_samples).  All of a
// thread's places in it are derived HERE from the thread index the kernel gives (fe400_kernel: threadIdx.x;
// fe400_fused_kernel: an opaque copy, see there).
struct Lane {
    int n2;                 // 25-point stage: lane (gl, n2) of the wave
    int wv, lane;           // wave, lane: the wave owns frames f0 + 4 wv .. f0 + 4 wv + 3
    int gl;                 // frame within the wave (== g & 3)
    float* are_w;           // this wave's 52 real rows (later: its 4 power rows)
    float* aim_w;           // this wave's 48 imaginary rows (first: its 640 samples)
    int g3l, k13;           // 16-point stage: lane = row (g3l, k13) of the wave's 52
    bool row_ok;
    int g3;                 // frame within the tile
};
__device__ __forceinline__ Lane lane_of(int tid, float* smem) {
    Lane t;
    t.n2 = tid & 15;
    t.wv = tid >> 6; t.lane = tid & 63;
    t.gl = t.lane >> 4;
    t.are_w = smem + O_ARE + t.wv * RE_W;
    t.aim_w = smem + O_AIM + t.wv * IM_W;
    t.g3l = t.lane / 13; t.k13 = t.lane - t.g3l * 13;
    t.row_ok = t.lane < WROWS;
    t.g3 = 4 * t.wv + t.g3l;
    return t;
}

// ---------------- tables this thread needs in registers (L2 hits; issued before anything waits)
__device__ __forceinline__ void load_window(const Fe400Args& a, const Lane& t, float (&wreg)[25]) {
#pragma unroll
    for (int n1 = 0; n1 < 25; ++n1) wreg[n1] = a.win_tw[16 * n1 + t.n2];
}

// sparse mel row of this thread (m, frame group): its descriptor now, its <= 14 weights behind the 25-point stage's
// operand reads -- two dependent L2 round trips that used to sit, exposed, in front of the mel loop
struct MelRow { int mm, mg, ms, mo, mcnt; };          // filter, frame group (3: idle lanes of the last wave); first bin, offset of the weights, their count
__device__ __forceinline__ MelRow load_mel_row(const Fe400Args& a, int tid) {
    MelRow r = {tid % NM, tid / NM, 0, 0, 0};
    if (r.mg < 3) {
        r.ms = a.mel_start[r.mm];
        r.mo = a.mel_off[r.mm];
        r.mcnt = a.mel_off[r.mm + 1] - r.mo;
    }
    return r;
}

// ---------------- samples: reflect padding of the pre-emphasised signal (np.pad(y_preem, 200, 'reflect'))
// The amplitude normalisation (audio_lib.py:125-126: y *= norm / mean|y|) is linear all the way to the power
// spectrum, so it is applied as a dB offset once mean|y| is known.
// The 640 samples under the wave's 4 frames and their predecessors are requested (the caller may do other work while
// they are in flight) ...
__device__ __forceinline__ void load_samples(const float* x, int L, const Lane& t, int f0, float (&cur)[10], float (&prv)[10]) {
    const int lane = t.lane;
    const int base = (f0 + 4 * t.wv) * HOP - HALF;
    const bool interior = base >= 1 && base + WSPAN <= L;   // wave-uniform: no reflection, no clamping
    if (interior) {
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            cur[u] = x[base + lane + 64 * u];
            prv[u] = x[base + lane + 64 * u - 1];
        }
    } else {
#pragma unroll
        for (int u = 0; u < 10; ++u) {
            const int idx = base + lane + 64 * u;
            int j = idx < 0 ? -idx : (idx >= L ? 2 * (L - 1) - idx : idx);
            j = min(max(j, 0), L - 1);
            cur[u] = x[j];
            prv[u] = j > 0 ? x[j - 1] : 0.0f;               // lfilter's zero initial state: y[0] = x[0]
        }
    }
}

// ... and, once they are here, stored pre-emphasised into the wave's sample buffer (its imaginary rows).  With ASUM:
// returns this thread's share of sum|x| over the samples [alo, ahi) -- the caller gives hops that are the tile's OWN,
// so that every sample of the utterance is counted once.
template <bool ASUM>
__device__ __forceinline__ float store_samples(const Fe400Args& a, const Lane& t, int L, int f0, const float (&cur)[10],
                                               const float (&prv)[10], int alo, int ahi) {
    float* const xs = t.aim_w;
    const int lane = t.lane;
    const int base = (f0 + 4 * t.wv) * HOP - HALF;
    const float pe = a.pre_emph;
    float asum = 0.0f;
#pragma unroll
    for (int u = 0; u < 10; ++u) {
        const int i = lane + 64 * u;
        const int idx = base + i;
        // beyond the reflected tail (idx >= L + 200) no frame of this utterance reads
        xs[i] = idx < L + HALF ? cur[u] - pe * prv[u] : 0.0f;
        if constexpr (ASUM) {
            if (idx >= alo && idx < ahi) asum += fabsf(cur[u]);
        }
    }
    return asum;
}

// (no barrier: the wave's power rows go over its OWN real rows, all of which are in its registers by now)
// power tile: bin k1 + 25 k2 directly for k2 <= 7 (and 200 = 0 + 25 * 8); the bins with residue 13..24 are the
// mirror images 400 - k of the outputs with k2 >= 8 (hermitian symmetry, fe_dft400.h bin_of).  With EXTREMES: the
// power's max / min over the frames that exist go into pmax / pmin.
template <bool EXTREMES>
__device__ __forceinline__ void store_power_rows(float* smem, const Lane& t, int f0, int F, const float (&pw)[16], float& pmax, float& pmin) {
    const int k13 = t.k13, g3 = t.g3;
    const bool row_ok = t.row_ok;
    const bool frame_ok = row_ok && (f0 + g3 >= 0) && (f0 + g3 < F);
    if (row_ok) {
        float* pg = smem + O_ARE + g3 * PP;
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) pg[k13 + 25 * k2] = pw[k2];
        if (k13 == 0) pg[200] = pw[8];
        else {
#pragma unroll
            for (int k2 = 8; k2 < 16; ++k2) pg[400 - 25 * k2 - k13] = pw[k2];
        }
        if constexpr (EXTREMES) {
            if (frame_ok) {
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2) { pmax = fmaxf(pmax, pw[k2]); pmin = fminf(pmin, pw[k2]); }
                if (k13 == 0) { pmax = fmaxf(pmax, pw[8]); pmin = fminf(pmin, pw[8]); }
                else {
#pragma unroll
                    for (int k2 = 8; k2 < 16; ++k2) { pmax = fmaxf(pmax, pw[k2]); pmin = fminf(pmin, pw[k2]); }
                }
            }
        }
    }
}

// ---------------- sparse mel: weights beyond the filter's own count are zeroed (the loads beside the 25-point stage clamp their index)
__device__ __forceinline__ void mask_mel_weights(float (&mw_)[14], int mcnt) {
#pragma unroll
    for (int j = 0; j < 14; ++j) mw_[j] = j < mcnt ? mw_[j] : 0.0f;
}

// ============================================================================================================
// THE FIVE STATISTICS (max / min of the power, max / min of the mel power, sum|x|): of a tile, and of an utterance.
__device__ __forceinline__ void wave_reduce5(float& pmx, float& pmn, float& mmx, float& mmn, float& as) {
    pmx = vc::wave_max(pmx); pmn = vc::wave_min(pmn);
    mmx = vc::wave_max(mmx); mmn = vc::wave_min(mmn);
    as = vc::wave_sum(as);
}

// A tile's statistics: every wave reduces its own and leaves them at scw[5 wv ..]; after a workgroup barrier (the
// caller's: the one-launch form drains stores in front of it) ...
__device__ __forceinline__ void tile_stats_partials(float* scw, int tid, float& pmax, float& pmin, float& mmax, float& mmin, float& asum) {
    wave_reduce5(pmax, pmin, mmax, mmin, asum);
    const int w = tid >> 6;
    if ((tid & 63) == 0) { scw[w * 5 + 0] = pmax; scw[w * 5 + 1] = pmin; scw[w * 5 + 2] = mmax; scw[w * 5 + 3] = mmin; scw[w * 5 + 4] = asum; }
}
// ... thread 0 folds the other waves' into its own, in wave order.
__device__ __forceinline__ void tile_stats_fold(const float* scw, float& pmax, float& pmin, float& mmax, float& mmin, float& asum) {
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) {
        pmax = fmaxf(pmax, scw[i * 5 + 0]); pmin = fminf(pmin, scw[i * 5 + 1]);
        mmax = fmaxf(mmax, scw[i * 5 + 2]); mmin = fminf(mmin, scw[i * 5 + 3]);
        asum += scw[i * 5 + 4];
    }
}

// An utterance's statistics from its nt tile records (8 floats each, from recs on): lane t, t + 64, ... of ONE wave, then
// wave_reduce5.  Every reader of an utterance's records goes through this walk -- the feature pass (plain loads), the
// one-launch form's last arriver and its no-wait path (SC1 loads) -- so all of them sum in the same order.
template <bool SC1>
__device__ __forceinline__ void walk_records(const float* recs, int nt, int lane, float& pmx, float& pmn, float& mmx, float& mmn, float& as) {
    pmx = NEG_INF; pmn = POS_INF; mmx = NEG_INF; mmn = POS_INF; as = 0.0f;
    for (int t = lane; t < nt; t += 64) {
        const float* s = recs + (size_t)t * 8;
        if constexpr (SC1) {
            pmx = fmaxf(pmx, ld_sc1(s + 0)); pmn = fminf(pmn, ld_sc1(s + 1));
            mmx = fmaxf(mmx, ld_sc1(s + 2)); mmn = fminf(mmn, ld_sc1(s + 3));
            as += ld_sc1(s + 4);
        } else {
            pmx = fmaxf(pmx, s[0]); pmn = fminf(pmn, s[1]);
            mmx = fmaxf(mmx, s[2]); mmn = fminf(mmn, s[3]);
            as += s[4];
        }
    }
}

// ============================================================================================================
// THE UTTERANCE'S CONSTANTS, by the lanes of wave 0 (tid < 64), into sc[0..8]: from the utterance's five statistics
// and frame 0's mel values v0 = mel0[tid], v1 = mel0[79 - tid] (tid < 40; anything finite elsewhere).
__device__ __forceinline__ void utterance_constants(const Fe400Args& a, float* sc, int tid, int L, float pmx, float pmn, float mmx,
                                                    float mmn, float as, float v0, float v1) {
    // amplitude normalisation as dB offsets: c = norm / mean|x| -> + 20 log10 c on the power dB, + 40 log10 c on
    // the mel dB; then the amin clamps (10 log10 1e-10 = 20 log10 1e-5 = -100 dB) and top_db = 80
    float offp = 0.0f;
    if (a.amp_norm != 1.0f) offp = 2.0f * DB10 * __log2f(a.amp_norm / (as / (float)L));
    const float offm = 2.0f * offp;
    // (the same two functions the elements go through in finish_tile: the utterance's minimum then maps to exactly 0)
    const float pfloor = fmaxf(pow_db_clipped(pmx, offp, -100.0f) - 80.0f, -100.0f);
    const float mfloor = fmaxf(mel_db_clipped(mmx, offm, -100.0f) - 80.0f, -100.0f);
    const float pmin_c = pow_db_clipped(pmn, offp, pfloor), mmin_c = mel_db_clipped(mmn, offm, mfloor);
    // the min shift and the scale are skipped at factor 1.0 (audio_lib.py:230-235)
    const bool pn = a.p_norm != 1.0f, mn = a.m_norm != 1.0f;
    if (tid == 0) {
        sc[0] = offp; sc[1] = pfloor;
        sc[2] = pn ? a.p_norm : 1.0f;
        sc[8] = pn ? pmin_c : 0.0f;
        sc[3] = offm; sc[4] = mfloor;
        sc[5] = mn ? a.m_norm : 1.0f;
        sc[6] = mn ? mmin_c : 0.0f;
    }
    // frame 0's first cepstral coefficient (audio_lib.py:221), summed exactly like the tile's own coefficient 0 in
    // finish_tile so that frame 0's own value cancels to 0
    float c00 = 0.0f;
    if (a.first_mfcc) {
        const float d0 = mel_db_clipped(v0, offm, mfloor), d1 = mel_db_clipped(v1, offm, mfloor);
        const float s0 = d0 + d1;
        const float dc = a.dct_half[0];                     // row 0 is constant: 1 / sqrt(80)
        float acc4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s0), j));
            acc4[j & 3] = fmaf(dc, sj, acc4[j & 3]);
        }
        c00 = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
    }
    if (tid == 0) sc[7] = c00;
}

// ============================================================================================================
// THE OUTPUT TAIL.  Thread tid < 240 computes coefficient tid / 6 of frames tid % 6, + 6, + 12 of the tile.
// DCT basis row of this thread's coefficient (rows of librosa.filters.dct(40, 80), first half): requested early, used
// four phases into finish_tile
__device__ __forceinline__ void load_dct_row(const Fe400Args& a, int tid, float (&drow)[NH]) {
    const int ci = tid / 6;
    if (tid < 240) {
#pragma unroll
        for (int j = 0; j < NH; j += 4) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(a.dct_half + ci * NH + j);
            drow[j] = d[0]; drow[j + 1] = d[1]; drow[j + 2] = d[2]; drow[j + 3] = d[3];
        }
    }
}

// From the power tile and the constants in sc[0..8] (a workgroup barrier behind both) to the 14 output rows from frame
// fo on.  mel_power(gg, mm) gives the mel power of tile frame gg, filter mm: the feature pass computes it from the power
// tile, the one-launch form kept it in the mel tile, where its dB value replaces it.
template <class MelPower>
__device__ __forceinline__ void finish_tile(const Fe400Args& a, float* smem, int tid, size_t row0, int fo, int F, const float (&drow)[NH],
                                            MelPower mel_power) {
    const float* const Pt = smem + O_ARE;
    float* const Mc = smem + O_MC;
    float* const Mf = smem + O_MF;
    float* const SD = smem + O_SD;
    const float* const sc = smem + O_SC;
    const float offp = sc[0], pfloor = sc[1], pS = sc[2], pM = sc[8], offm = sc[3], mfloor = sc[4], mS = sc[5], mM = sc[6],
                c00 = sc[7];
    const int nvalid = min(GO, F - fo);             // output frames that exist
    const int nrows = min(GO, a.out_rows - fo);     // output rows of the buffers (the rest of them: zeros); <= 0 past out_rows
    const int mm = tid % NM, mg = tid / NM;
    const int ci = tid / 6, cf = tid - ci * 6;      // coefficient, frame phase (tid < 240)

    // ---------------- P_dB: thread k < 201 walks column k of tile rows 1..14 (every LDS address an immediate, the
    // global stores of a wave are consecutive floats)
    if (tid < NB) {
        float* o = a.pow_db + (row0 + fo) * NB + tid;
        const float* p = Pt + PP + tid;
        const bool clip = a.clip != 0;
#pragma unroll
        for (int gg = 0; gg < GO; ++gg) {
            float w = pS * (pow_db_clipped(p[gg * PP], offp, pfloor) - pM);
            if (clip) w = fminf(fmaxf(w, -1.0f), 1.0f);
            if (gg < nrows) o[gg * NB] = gg < nvalid ? w : 0.0f;
        }
    }
    // ---------------- mel power -> dB of the "amplitude" (quirk) -> top_db clip: all 16 frames (DCT halo)
    if (mg < 3) {
        for (int gg = mg; gg < G; gg += 3) Mc[gg * NM + mm] = mel_db_clipped(mel_power(gg, mm), offm, mfloor);
    }
    __syncthreads();
    // ---------------- M_dB out (float4 rows) and the sum / difference halves for the DCT
    {
        const bool clip = a.clip != 0;
        f32x4* o = reinterpret_cast<f32x4*>(a.mel_db + (row0 + fo) * NM);
        for (int i = tid; i < nrows * (NM / 4); i += NT) {
            f32x4 v = *reinterpret_cast<const f32x4*>(Mc + NM + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float w = mS * (v[e] - mM);
                if (clip) w = fminf(fmaxf(w, -1.0f), 1.0f);
                v[e] = 4 * i < nvalid * NM ? w : 0.0f;
            }
            o[i] = v;
        }
        for (int i = tid; i < G * NH; i += NT) {
            const int gg = i / NH, j = i - gg * NH;
            const float lo = Mc[gg * NM + j], hi = Mc[gg * NM + NM - 1 - j];
            SD[gg * NM + j] = lo + hi;
            SD[gg * NM + NH + j] = lo - hi;
        }
    }
    __syncthreads();
    // ---------------- DCT-II: coefficient ci (even: sums, odd: differences), frames cf, cf + 6, cf + 12
    if (tid < 240) {
        const float norm = a.mfcc_norm;
        for (int gg = cf; gg < G; gg += 6) {
            const f32x4* sd = reinterpret_cast<const f32x4*>(SD + gg * NM + (ci & 1) * NH);
            float acc4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < NH / 4; ++j) {
                const f32x4 s = sd[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc4[e] = fmaf(drow[4 * j + e], s[e], acc4[e]);
            }
            float acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
            if (ci == 0) acc -= c00;
            if (norm != 1.0f) acc *= norm;
            Mf[gg * NC + ci] = acc;
        }
    }
    __syncthreads();
    // ---------------- [MFCC | delta] out (audio_lib.py:226-228, 238): delta = 2 (M[t+1] - M[t-1]), 0 at both ends
    {
        const bool clip = a.clip != 0;
        const int mw = a.deriv ? 2 * NC : NC;
        f32x4* o = reinterpret_cast<f32x4*>(a.mfcc + (row0 + fo) * mw);
        const int per_row = mw / 4;
        for (int i = tid; i < nrows * per_row; i += NT) {
            const int gg = i / per_row, c = 4 * (i - gg * per_row);
            const int f = fo + gg;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (f < F) {
                if (c < NC) {
                    v = *reinterpret_cast<const f32x4*>(Mf + (gg + 1) * NC + c);
                } else if (f >= 1 && f <= F - 2) {
                    const f32x4 nx = *reinterpret_cast<const f32x4*>(Mf + (gg + 2) * NC + (c - NC));
                    const f32x4 pv = *reinterpret_cast<const f32x4*>(Mf + gg * NC + (c - NC));
                    v = 2.0f * (nx - pv);
                }
                if (clip) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf(v[e], -1.0f), 1.0f);
                }
            }
            o[i] = v;
        }
    }
}

// padding rows of a ragged batch (a tile whose frames lie past the utterance's last): zeros
__device__ __forceinline__ void zero_tile_rows(const Fe400Args& a, int tid, size_t row0, int fo) {
    const int nrows = min(GO, a.out_rows - fo);
    const int mw = a.deriv ? 2 * NC : NC;
    float* o1 = a.mfcc + (row0 + fo) * mw;
    float* o2 = a.mel_db + (row0 + fo) * NM;
    float* o3 = a.pow_db + (row0 + fo) * NB;
    for (int i = tid; i < nrows * mw; i += NT) o1[i] = 0.0f;
    for (int i = tid; i < nrows * NM; i += NT) o2[i] = 0.0f;
    for (int i = tid; i < nrows * NB; i += NT) o3[i] = 0.0f;
}

// ============================================================================================================
// TWO-LAUNCH FORM: the statistics pass (STATS) and the feature pass.
template <bool STATS>
__global__ void __launch_bounds__(NT, 4)
fe400_kernel(Fe400Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const sc = smem + O_SC;
    const float* const Pt = smem + O_ARE;               // power tile: row g at Pt + g * PP (4 rows per wave region)

    const int tid = threadIdx.x, b = blockIdx.y;
    const int L = utt_len(a, b);
    const int F = 1 + L / HOP;
    // first transformed frame of the tile (pass 2: one halo frame ahead of the first output frame)
    const int fo = (STATS ? G : GO) * (int)blockIdx.x;          // first frame this block is responsible for
    const int f0 = STATS ? fo : fo - 1;
    const size_t row0 = (size_t)b * a.out_rows;          // the output arrays hold out_rows <= max_frames rows per utterance

    if (fo >= F) {
        if constexpr (STATS) {
            if (tid == 0) {
                float* s = a.stats + ((size_t)b * a.nt1 + blockIdx.x) * 8;
                s[0] = NEG_INF; s[1] = POS_INF; s[2] = NEG_INF; s[3] = POS_INF; s[4] = 0.0f;
            }
        } else {
            zero_tile_rows(a, tid, row0, fo);
        }
        return;
    }

    const Lane t = lane_of(tid, smem);
    float wreg[25];
    load_window(a, t, wreg);
    const MelRow mr = load_mel_row(a, tid);

    // ---------------- pass 2, wave 0: the utterance's tile records and frame 0's mel row are requested FIRST, so that
    // their round trips run beside the block's sample loads; the constants are computed while the samples are in flight
    float r_pmx = NEG_INF, r_pmn = POS_INF, r_mmx = NEG_INF, r_mmn = POS_INF, r_as = 0.0f, r_v0 = 1.0f, r_v1 = 1.0f;
    if constexpr (!STATS) {
        if (tid < 64) {
            walk_records<false>(a.stats + (size_t)b * a.nt1 * 8, (F + G - 1) / G, tid, r_pmx, r_pmn, r_mmx, r_mmn, r_as);
            if (a.first_mfcc && tid < NH) {
                r_v0 = a.mel0[(size_t)b * NM + tid];
                r_v1 = a.mel0[(size_t)b * NM + NM - 1 - tid];
            }
        }
    }
    const float* x = a.wav + (size_t)b * a.wav_stride;
    float cur[10], prv[10];
    load_samples(x, L, t, f0, cur, prv);
    if constexpr (!STATS) {
        if (tid < 64) {
            wave_reduce5(r_pmx, r_pmn, r_mmx, r_mmn, r_as);
            utterance_constants(a, sc, tid, L, r_pmx, r_pmn, r_mmx, r_mmn, r_as, r_v0, r_v1);
        }
    }
    // sum|x| of the wave's OWN hops [fw*80, (fw+4)*80): every sample of the utterance counted once
    const int fw = f0 + 4 * t.wv;                       // first frame of the wave
    float asum = store_samples<STATS>(a, t, L, f0, cur, prv, fw * HOP, min((fw + 4) * HOP, L));

    // The two DFT stages stand in each kernel (here and in fe400_fused_kernel), not in a helper: every one of their
    // products feeds a sum the compiler contracts to an FMA, and WHICH of two products of a sum gets fused follows
    // the operand order the optimiser settles on -- inside a helper it settles on another one (measured: 28 of a
    // block's LDS row stores and 3 of its power stores then hold other expressions; the features move by up to
    // 2.4e-6).  Both copies must stay textually equal: the forms agree to rounding only as long as they are.
    // The way out is vcfe::pinned of fe_dft400.h (the vocoder's forward kernels are on it): read the choices these two
    // copies were compiled to out of their ISA, write them down as fmaf, and one definition serves both.
    float mw_[14], pw[16];
#pragma unroll
    for (int j = 0; j < 14; ++j) mw_[j] = 0.0f;
    // ---------------- steps 1 + 2: lane (gl, n2): real 25-point DFT over n1, twiddle W400^(n2 k1).  Wave-local: the
    // wave's own LDS writes above are ordered before these reads, and every read of the samples is issued before the
    // row stores that overwrite them (same wave, in order).
    {
        const float* xp = t.aim_w + t.gl * HOP + t.n2;
        float v[25], ar[13], ai[13];
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) v[n1] = xp[16 * n1] * wreg[n1];
        // twiddles and this thread's mel weights: requested here (L2 hits), consumed behind the 25-point transform
        if (mr.mg < 3) {
#pragma unroll
            for (int j = 0; j < 14; ++j) mw_[j] = a.mel_w[mr.mo + min(j, max(mr.mcnt - 1, 0))];
        }
        float twr[13], twi[13];
#pragma unroll
        for (int k1 = 1; k1 < 13; ++k1) { twr[k1] = a.win_tw[400 + k1 * 16 + t.n2]; twi[k1] = a.win_tw[608 + k1 * 16 + t.n2]; }
        vcfe::rdft25_13(v, ar, ai);
        // the reads of v[] above must have RETURNED before any row store may land on the sample buffer: the compiler
        // orders them (ar / ai depend on v), the LDS unit executes a wave's operations in order
        const int r0 = t.gl * 13, i0 = t.gl * 12 - 1;
        t.are_w[(r0)*RP + t.n2] = ar[0];                // ai[0] == 0: not stored
#pragma unroll
        for (int k1 = 1; k1 < 13; ++k1) {
            vcfe::cmul(ar[k1], ai[k1], twr[k1], twi[k1]);
            t.are_w[(r0 + k1) * RP + t.n2] = ar[k1];
            t.aim_w[(i0 + k1) * RP + t.n2] = ai[k1];
        }
    }
    // ---------------- step 3: lane = row (g3l, k13) of the wave's 52: complex 16-point DFT over n2 -> |Y|^2
    {
        float zr[16], zi[16], yr[16], yi[16];
        const int r = t.row_ok ? t.lane : 0;
        const bool has_im = t.row_ok && t.k13 > 0;
        const int ri = has_im ? t.g3l * 12 + t.k13 - 1 : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 vr = *reinterpret_cast<const f32x4*>(t.are_w + r * RP + 4 * q);
            const f32x4 vi = *reinterpret_cast<const f32x4*>(t.aim_w + ri * RP + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) { zr[4 * q + e] = vr[e]; zi[4 * q + e] = has_im ? vi[e] : 0.0f; }
        }
        vcfe::cdft16(zr, zi, yr, yi);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) pw[k2] = yr[k2] * yr[k2] + yi[k2] * yi[k2];
    }
    float drow[STATS ? 1 : NH];
    if constexpr (!STATS) load_dct_row(a, tid, drow);
    float pmax = NEG_INF, pmin = POS_INF;
    store_power_rows<STATS>(smem, t, f0, F, pw, pmax, pmin);
    mask_mel_weights(mw_, mr.mcnt);

    if constexpr (STATS) {
        float mmax = NEG_INF, mmin = POS_INF;
        __syncthreads();                                // power tile complete
        if (mr.mg < 3) {
            for (int gg = mr.mg; gg < G; gg += 3) {
                const float acc = mel_dot(Pt + gg * PP + mr.ms, mw_);
                if (f0 + gg < F) { mmax = fmaxf(mmax, acc); mmin = fminf(mmin, acc); }
                if (f0 + gg == 0) a.mel0[(size_t)b * NM + mr.mm] = acc;
            }
        }
        tile_stats_partials(sc, tid, pmax, pmin, mmax, mmin, asum);
        __syncthreads();
        if (tid == 0) {
            tile_stats_fold(sc, pmax, pmin, mmax, mmin, asum);
            float* s = a.stats + ((size_t)b * a.nt1 + blockIdx.x) * 8;
            s[0] = pmax; s[1] = pmin; s[2] = mmax; s[3] = mmin; s[4] = asum;
        }
    } else {
        __syncthreads();                                // power tile + constants
        finish_tile(a, smem, tid, row0, fo, F, drow, [&](int gg, int) { return mel_dot(Pt + gg * PP + mr.ms, mw_); });
    }
}


// ============================================================================================================
// ONE-LAUNCH FORM: every frame transformed once.
//
// The two-pass form transforms every frame twice because the normalisations need the utterance's extremes before a
// single output value can be written.  Here a block transforms its 16 frames (14 outputs + one halo frame each side),
// keeps the power tile and the mel-power tile in LDS, PUBLISHES its tile record (max / min of the power and of the mel
// power, sum|x| of its own hops; the tile holding frame 0 also that frame's mel row), and then waits until all tiles of
// ITS OWN UTTERANCE have published -- a per-utterance counter, not a grid barrier -- before it finishes dB / DCT /
// delta from LDS and stores.  Blocks whose frames lie past `out_rows` only publish and leave.
//
// Hand-off (cdna_hip_programming.md Guideline 16, form R1): record words are write-through (sc1) stores, every storing
// wave drains them (vmcnt(0)), a workgroup barrier, then ONE lane adds to the utterance's counter (agent scope).  The tile
// whose add completes the count reduces the utterance's records to one line (write-through, drained) and raises the
// utterance's READY word; the consumers poll that word relaxed from one lane and read the line with sc1 loads only (they
// bypass this CU's L1: nothing here can be stale; every utterance's records, its line, its counter and its READY word
// sit on cache lines of their own).  The counters and READY words are the first block of the caller's workspace, zeroed
// by a small kernel on the launch's stream right before this one: no state outlives a launch or is shared by two of them,
// so a captured graph replays correctly and launches of one plan with separate workspaces may run concurrently.
//
// Forward progress without any assumption about dispatch order or residency: a publisher never waits, and a waiter
// whose poll runs out (4 ms; an utterance's tiles normally arrive within microseconds of each other because workgroups
// of one utterance are neighbours in the grid) stops waiting and computes the utterance's records ITSELF -- it walks
// all tiles of the utterance through the same transform code, writes their records (the same values their owners
// write), re-transforms its own tile to restore the LDS tiles, and goes on.  Slow, never wrong, never stuck.
constexpr unsigned FUSED_SPIN_LIMIT = 4000;          // x (s_sleep 24 + one L2 round trip) ~ 4 ms
// One counter per 256 bytes: with the 32 counters of a batch in ONE cache line every arrival and every poll of ~1,000
// resident blocks went through one L2 channel (a word serves ~88 requests per microsecond): blocks waited a median of
// 69,000 cycles for their utterance and the launch took 103 us (profiles/r03).
constexpr int FCOUNT_PITCH = 64;                     // unsigned words

__global__ void __launch_bounds__(NT, 4)
fe400_fused_kernel(Fe400Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const sc = smem + O_SC;
    const float* const Pt = smem + O_ARE;               // power tile: row g at Pt + g * PP (4 rows per wave region)
    float* const Mc = smem + O_MC;                      // [G][80]  mel POWER until the utterance's constants are known, then clipped mel dB

    const int tid = threadIdx.x, b = blockIdx.y;
    const int L = utt_len(a, b);
    const int F = 1 + L / HOP;
    const int own = blockIdx.x;
    const int fo_own = GO * own;
    const size_t row0 = (size_t)b * a.out_rows;

    if (fo_own >= F) {                                  // (such tiles publish nothing)
        zero_tile_rows(a, tid, row0, fo_own);
        return;
    }
    const int nt_b = (F + GO - 1) / GO;                 // tiles of this utterance that publish
    const bool has_out = fo_own < a.out_rows;
    float* const recs = a.fstats + (size_t)b * a.fstride;
    typedef __attribute__((address_space(1))) unsigned gu32;
    gu32* const cnt = (gu32*)(uintptr_t)(a.fcount + (size_t)b * FCOUNT_PITCH);

    const float* x = a.wav + (size_t)b * a.wav_stride;

    // mode 0: own tile (publish, wait); 1: walking the utterance's tiles after a poll ran out; 2: own tile again
    int mode = 0, cur = own;
    for (;;) {
        const int fo = GO * cur, f0 = fo - 1;
        // Every per-thread index of the transform is derived INSIDE the loop from an opaque copy of the thread index: the
        // loop runs once unless a poll ran out, but hoisted out of it the tables, LDS addresses and row maps (loop
        // invariants) stay live through the wait and the gather and the kernel spills 60 registers.  For the same
        // reason the window, the twiddles and the mel weights are NOT kept across iterations.
        int tid_l = threadIdx.x;
        asm volatile("" : "+v"(tid_l));
        const Lane t = lane_of(tid_l, smem);
        const MelRow mr = load_mel_row(a, tid_l);
        float wreg[25];
        load_window(a, t, wreg);
        float curv[10], prv[10];
        load_samples(x, L, t, f0, curv, prv);
        // sum|x| of the tile's OWN hops [fo*80, (fo+14)*80), every sample of the utterance counted once: this wave's
        // share is the part of its four frames' hops that lies inside
        const int fw = f0 + 4 * t.wv;
        float asum = store_samples<true>(a, t, L, f0, curv, prv, max(fw, fo) * HOP, min(min((fw + 4), fo + GO) * HOP, L));
        // ---------------- the two DFT stages: the text of fe400_kernel's (why they are not in a helper: see there)
        float mw_[14], pw[16];
#pragma unroll
        for (int j = 0; j < 14; ++j) mw_[j] = 0.0f;
        {
            const float* xp = t.aim_w + t.gl * HOP + t.n2;
            float v[25], ar[13], ai[13];
#pragma unroll
            for (int n1 = 0; n1 < 25; ++n1) v[n1] = xp[16 * n1] * wreg[n1];
            if (mr.mg < 3) {
#pragma unroll
                for (int j = 0; j < 14; ++j) mw_[j] = a.mel_w[mr.mo + min(j, max(mr.mcnt - 1, 0))];
            }
            float twr[13], twi[13];
#pragma unroll
            for (int k1 = 1; k1 < 13; ++k1) { twr[k1] = a.win_tw[400 + k1 * 16 + t.n2]; twi[k1] = a.win_tw[608 + k1 * 16 + t.n2]; }
            vcfe::rdft25_13(v, ar, ai);
            const int r0 = t.gl * 13, i0 = t.gl * 12 - 1;
            t.are_w[(r0)*RP + t.n2] = ar[0];                // ai[0] == 0: not stored
#pragma unroll
            for (int k1 = 1; k1 < 13; ++k1) {
                vcfe::cmul(ar[k1], ai[k1], twr[k1], twi[k1]);
                t.are_w[(r0 + k1) * RP + t.n2] = ar[k1];
                t.aim_w[(i0 + k1) * RP + t.n2] = ai[k1];
            }
        }
        {
            float zr[16], zi[16], yr[16], yi[16];
            const int r = t.row_ok ? t.lane : 0;
            const bool has_im = t.row_ok && t.k13 > 0;
            const int ri = has_im ? t.g3l * 12 + t.k13 - 1 : 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 vr = *reinterpret_cast<const f32x4*>(t.are_w + r * RP + 4 * q);
                const f32x4 vi = *reinterpret_cast<const f32x4*>(t.aim_w + ri * RP + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) { zr[4 * q + e] = vr[e]; zi[4 * q + e] = has_im ? vi[e] : 0.0f; }
            }
            vcfe::cdft16(zr, zi, yr, yi);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) pw[k2] = yr[k2] * yr[k2] + yi[k2] * yi[k2];
        }
        float pmax = NEG_INF, pmin = POS_INF;
        store_power_rows<true>(smem, t, f0, F, pw, pmax, pmin);
        __syncthreads();                                // power tile complete; every wave is past its imaginary rows
        // ---------------- mel power of all 16 frames -> LDS; extremes; frame 0's row
        mask_mel_weights(mw_, mr.mcnt);
        float mmax = NEG_INF, mmin = POS_INF;
        if (mr.mg < 3) {
            for (int gg = mr.mg; gg < G; gg += 3) {
                const float acc = mel_dot(Pt + gg * PP + mr.ms, mw_);
                Mc[gg * NM + mr.mm] = acc;
                if (f0 + gg >= 0 && f0 + gg < F) { mmax = fmaxf(mmax, acc); mmin = fminf(mmin, acc); }
                if (f0 + gg == 0 && mode != 2) st_sc1(a.mel0 + (size_t)b * NM + mr.mm, acc);
            }
        }
        tile_stats_partials(sc + 16, tid_l, pmax, pmin, mmax, mmin, asum);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (frame 0's mel row: every storing wave drains)
        __syncthreads();
        if (mode == 2) break;                           // own tiles restored; the records are all in memory
        if (tid == 0) {
            tile_stats_fold(sc + 16, pmax, pmin, mmax, mmin, asum);
            float* r8 = recs + (size_t)cur * 8;
            st_sc1(r8 + 0, pmax); st_sc1(r8 + 1, pmin); st_sc1(r8 + 2, mmax); st_sc1(r8 + 3, mmin); st_sc1(r8 + 4, asum);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (mode == 0 && t.wv == 0) {
            // Arrival (wave 0).  The LAST tile of the utterance to arrive reduces the records to one line and raises the
            // utterance's READY word; everybody else polls that word and reads the one line (58 records gathered by
            // every block cost 7 k cycles of a 52 k-cycle block life and most of the L2 traffic the polls compete with).
            unsigned old = 0;
            if (t.lane == 0) old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
            if (old == (unsigned)(nt_b - 1)) {
                float r_pmx, r_pmn, r_mmx, r_mmn, r_as;
                walk_records<true>(recs, nt_b, t.lane, r_pmx, r_pmn, r_mmx, r_mmn, r_as);
                wave_reduce5(r_pmx, r_pmn, r_mmx, r_mmn, r_as);
                if (t.lane == 0) {
                    float* s8 = recs + a.fstride - 32;
                    st_sc1(s8 + 0, r_pmx); st_sc1(s8 + 1, r_pmn); st_sc1(s8 + 2, r_mmx); st_sc1(s8 + 3, r_mmn); st_sc1(s8 + 4, r_as);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(cnt + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (t.lane == 0) {
                int ok = 1;
                if (has_out) {
                    ok = 0;
                    for (int spins = 0; spins < a.spin_limit; ++spins) {
                        if (__hip_atomic_load(cnt + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { ok = 1; break; }
                        __builtin_amdgcn_s_sleep(16);
                    }
                }
                reinterpret_cast<int*>(sc)[40] = ok;
            }
        }
        if (mode == 0) {
            if (!has_out) return;                       // statistics-only tile (frames past out_rows): published, done
            __syncthreads();
            if (reinterpret_cast<const int*>(sc)[40]) break;
            mode = 1; cur = 0;                          // the poll ran out: compute the utterance's records here
        } else {
            __syncthreads();                            // (sc is rewritten by the next tile)
            if (++cur == nt_b) { mode = 2; cur = own; }
        }
    }

    // ---------------- the utterance's constants (wave 0), from the published records: sc1 loads only
    // (everything below is addressed from an opaque copy of the thread index: left to itself the compiler computes the
    // output addresses of all phases BEFORE the tile loop and spills 64 registers to carry them across it)
    int tid_c = threadIdx.x;
    asm volatile("" : "+v"(tid_c));
    if (tid_c < 64) {
        float r_v0 = 1.0f, r_v1 = 1.0f;
        if (a.first_mfcc && tid_c < NH) {
            r_v0 = ld_sc1(a.mel0 + (size_t)b * NM + tid_c);
            r_v1 = ld_sc1(a.mel0 + (size_t)b * NM + NM - 1 - tid_c);
        }
        float pmx, pmn, mmx, mmn, as;
        if (mode == 2) {
            // this block computed the records itself (its poll ran out): the same walk and reduction as the last arriver's
            walk_records<true>(recs, nt_b, tid_c, pmx, pmn, mmx, mmn, as);
            wave_reduce5(pmx, pmn, mmx, mmn, as);
        } else {
            const float* s8 = recs + a.fstride - 32;     // the utterance's line, written by its last arriver
            pmx = ld_sc1(s8 + 0); pmn = ld_sc1(s8 + 1); mmx = ld_sc1(s8 + 2); mmn = ld_sc1(s8 + 3); as = ld_sc1(s8 + 4);
        }
        utterance_constants(a, sc, tid_c, L, pmx, pmn, mmx, mmn, as, r_v0, r_v1);
    }
    float drow[NH];
    load_dct_row(a, tid_c, drow);
    __syncthreads();                                    // constants
    // the mel power -> clipped dB in place: each thread the elements it wrote
    finish_tile(a, smem, tid_c, row0, fo_own, F, drow, [&](int gg, int mm) { return Mc[gg * NM + mm]; });
}

}  // namespace

int vc_fe400_fused_count_bytes(int batch) { return batch * FCOUNT_PITCH * 4; }
int vc_fe400_fused_stride(int max_frames) { return ((((max_frames + GO - 1) / GO) * 8 + 31) & ~31) + 32; }       // + the utterance's summary line
// (utterances up to ~36 s; longer ones would keep early tiles waiting for tiles many rounds of workgroups away)
bool vc_fe400_fused_ok(int max_frames) { return (max_frames + GO - 1) / GO <= 512; }

int vc_fe400_launch(const Fe400Args& a, int batch, int stage_mask, int fused, hipStream_t st) {
    const size_t lds = (size_t)LDS_FLOATS * 4;
    if (fused) {
        const int ntf = (a.max_frames + GO - 1) / GO;
        Fe400Args f = a;
        const int sl = vc::opt(vc::OPT_FE_FUSED_SPIN);          // tests: 0 = every waiting block takes the no-wait path
        f.spin_limit = sl >= 0 ? sl : (int)FUSED_SPIN_LIMIT;
        // every counter and READY word the launch polls starts at zero: a node of its own under graph capture, replayed
        // before the kernel (nothing is carried from one launch to the next; vc::zero_async, not hipMemsetAsync)
        VC_HIP_CHECK(vc::zero_async(a.fcount, (size_t)vc_fe400_fused_count_bytes(batch), st));
        hipLaunchKernelGGL(fe400_fused_kernel, dim3(ntf, batch), dim3(NT), lds, st, f);
        VC_HIP_CHECK(hipGetLastError());
        return VC_OK;
    }
    if (stage_mask & 2)
        hipLaunchKernelGGL(fe400_kernel<true>, dim3(a.nt1, batch), dim3(NT), lds, st, a);
    if (stage_mask & 4) {
        const int nt2 = (a.out_rows + GO - 1) / GO;    // tiles past the stored rows have nothing to write
        hipLaunchKernelGGL(fe400_kernel<false>, dim3(nt2, batch), dim3(NT), lds, st, a);
    }
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}
