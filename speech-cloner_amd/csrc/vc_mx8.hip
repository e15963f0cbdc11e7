// MX-FP8 inference of the decoder's filter banks and the projection behind them (include/vc_hip.h, "MX-FP8").
//
//   vc_mx8_quantize  bf16 / float32 [M, C] -> e4m3fn codes + one E8M0 scale per 32 channels (vc_mx8.h rule)
//   vc_mx8_conv      SAME convolution of MX operands on v_mfma_scale_f32_32x32x64_f8f6f4 (block-scaled fp8 MFMA,
//                    twice the bf16 matrix rate), float32 accumulation, folded-BN + relu epilogue, optionally
//                    max_pool(2, 1, same) and MX-FP8 output (the bank), or bf16 output (the projection)
//
// Work decomposition of mx8_conv_kernel: a workgroup (4 waves) computes 128 frames x two 128-channel groups; wave w
// owns channels (w & 1) * 64 .. + 63 of group 2 * gp + (w >> 1) over all 128 frames, as 2 x 4 tiles of 32 x 32
// (128 accumulator registers).  The weights are the A operand (channels on the accumulator registers, frames on the
// lanes), so a lane and lane ^ 32 together hold the 32 channels of one frame: one MX output block, whose amax takes one
// cross-lane exchange; the frame neighbour of max_pool(2, 1) is the next lane (or the next tile's lane 0).  With pool
// the row tiles advance by 127 frames, so every output frame's right neighbour is computed in the same wave.
// A group pair shares its SAME left padding (bank widths 2p+1 / 2p+2, or the two halves of one 256-channel filter), so
// the 128 + taps - 1 activation rows of a tile are staged in LDS once per slab of up to 256 channels (rows padded by
// 16 bytes: the 16 lanes of a ds_read_b128 phase hit 16 different bank groups) and read by all 4 waves for every tap;
// the K loop runs tap-major over 64-channel steps, unrolled by two over two register sets, so that the next step's
// weights (streamed from L2) and activation fragments (LDS) are in flight during the current step's 8 MFMAs.  Measured alternatives that were not faster: 256-frame tiles with
// one filter per workgroup (half the weight traffic), and weights two K steps ahead.
//
// Operand lane map of the 32x32x64 f8f6f4 form, pinned with exact integer data (tests/test_mx8_gpu.py, lane map):
// lane l (r = l & 31, h = l >> 5) holds row r of A (column r of B) at k = 16h .. 16h+15 in bytes 0..15 and
// k = 32 + 16h .. 32 + 16h + 15 in bytes 16..31; its scale byte is that of K block h (k = 32h .. 32h + 31) of row r.
#include <algorithm>
#include <cstdlib>
#include "vc_device.h"
#include "vc_mx8.h"

using vc::f32x16, vc::i32x8;

namespace {

constexpr int NT = 256;
constexpr int TILE = 128;            // frames per workgroup
constexpr int MAX_SPLIT = 4;

struct Mx8Args {
    const uint8_t* X;
    const uint8_t* Xs;
    int32_t M, T, Cin, n_groups;
    vc_mx8_group g[VC_MX8_MAX_GROUPS];
    const float* scale;
    const float* shift;
    int32_t act, pool, out_mode, n_out;
    void* C;
    uint8_t* Cs;
    float* ws;                       // split K: [ksplit][M][n_out] float32 partial sums
    int32_t ksplit;
};

__device__ __forceinline__ uint32_t bf16_rne(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// channels staged in LDS per pass: the largest of 256 / 192 / 128 / 64 that divides Cin
__host__ __device__ inline int slab_of(int Cin) {
    return Cin % 256 == 0 ? 256 : Cin % 192 == 0 ? 192 : Cin % 128 == 0 ? 128 : 64;
}
__host__ __device__ inline size_t lds_bytes(int Cin, int max_taps) {
    const int rows = TILE + max_taps;                  // + one all-zero row
    const int slab = slab_of(Cin);
    return (size_t)rows * (slab + 16) + (size_t)rows * (slab >> 5);
}

struct Frag {
    i32x8 v;
    int s;
};

// 32 bytes of one row at k0 (bytes 16h .. 16h+15 and 32+16h .. 32+16h+15 of the 64-wide step) and the scale of block h
__device__ __forceinline__ Frag load_frag(const uint8_t* row, const uint8_t* srow, int h) {
    const uint4 lo = *reinterpret_cast<const uint4*>(row + 16 * h);
    const uint4 hi = *reinterpret_cast<const uint4*>(row + 32 + 16 * h);
    Frag f;
    f.v = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    f.s = srow[h];
    return f;
}

__global__ void __launch_bounds__(NT, 1)
mx8_conv_kernel(Mx8Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_pairs = (a.n_groups + 1) >> 1;
    const int g0 = 2 * (n_pairs - 1 - (int)blockIdx.y);                     // widest pair first
    const int gi = g0 + (wid >> 1);
    const bool idle = gi >= a.n_groups;                 // odd group count: this wave stages and waits, computes nothing
    const vc_mx8_group gr = a.g[idle ? g0 : gi];
    const int pad_l = a.g[g0].pad_l;                    // shared by the pair
    const int max_taps = g0 + 1 < a.n_groups ? max(a.g[g0].taps, a.g[g0 + 1].taps) : a.g[g0].taps;
    const int ch0 = (wid & 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * (a.pool ? TILE - 1 : TILE);
    const int Cin = a.Cin, Kw = gr.taps * Cin;
    const int slab = slab_of(Cin), ncs = slab >> 6, nslab = Cin / slab;
    const int ks = blockIdx.z;
    const int sl0 = ks * nslab / a.ksplit, sl1 = (ks + 1) * nslab / a.ksplit;
    const int rows = TILE + max_taps - 1, rb = slab + 16, sb = slab >> 5;
    // [rows + 1][slab + 16] codes (16-byte pad: conflict-free row reads), then [rows + 1][slab / 32] scales; row `rows`
    // is all zero: the fragments of frames whose tap falls outside their window (SAME padding) are read from it
    uint8_t* const xl = smem;
    uint8_t* const sl_s = smem + (rows + 1) * rb;
    const uint8_t* W = reinterpret_cast<const uint8_t*>(gr.d_W);
    const uint8_t* Ws = reinterpret_cast<const uint8_t*>(gr.d_Ws);

    int tloc[4];
    bool live[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const int m = m0 + fb * 32 + r;
        live[fb] = m < a.M;
        tloc[fb] = live[fb] ? m % a.T : 0;
    }

    f32x16 acc[2][4];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[cb][fb][i] = 0.0f;

    auto load_w = [&](int sl, int j, int cc, Frag (&fa)[2]) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int n = ch0 + cb * 32 + r;
            const size_t k0 = (size_t)n * Kw + (size_t)j * Cin + sl * slab + cc * 64;
            fa[cb] = load_frag(W + k0, Ws + (k0 >> 5), h);
        }
    };

    const int nstep = idle ? 0 : gr.taps * ncs;         // K steps of this wave per slab: tap-major, 64 channels each
    for (int sl = sl0; sl < sl1; ++sl) {
        // stage rows m0 - pad_l .. + rows - 1 of the slab (zero outside [0, M)) and the zero row
        __syncthreads();
        const int cpr = slab >> 4;
        for (int i = tid; i < (rows + 1) * cpr; i += NT) {
            const int rr = i / cpr, c = i - rr * cpr, g = m0 - pad_l + rr;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (rr < rows && g >= 0 && g < a.M) v = *reinterpret_cast<const uint4*>(a.X + (size_t)g * Cin + sl * slab + c * 16);
            *reinterpret_cast<uint4*>(xl + rr * rb + c * 16) = v;
        }
        for (int i = tid; i < (rows + 1) * sb; i += NT) {
            const int rr = i / sb, q = i - rr * sb, g = m0 - pad_l + rr;
            sl_s[rr * sb + q] = (rr < rows && g >= 0 && g < a.M) ? a.Xs[(size_t)g * (Cin >> 5) + sl * sb + q] : (uint8_t)127;
        }
        __syncthreads();
        // two register sets, unrolled by two: step s + 1's weights (L2) and activations (LDS) are in flight while step
        // s's 8 MFMAs run.  Every load is unconditional (masked frames read the zero row, the last step reloads itself):
        // a load under a branch, or a rotation through register copies, made the compiler wait for loads it had just
        // issued before the MFMAs.
        auto load_x = [&](int s, Frag (&fx)[4]) {
            const int j = s / ncs, cc = s - j * ncs;
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const int t = tloc[fb] - pad_l + j;
                const int rr = (live[fb] && t >= 0 && t < a.T) ? fb * 32 + r + j : rows;
                fx[fb] = load_frag(xl + rr * rb + cc * 64, sl_s + rr * sb + cc * 2, h);
            }
        };
        auto mma = [&](const Frag (&fa)[2], const Frag (&fx)[4]) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb)
                    acc[cb][fb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[cb].v, fx[fb].v, acc[cb][fb], 0, 0,
                                                                                  0, fa[cb].s, 0, fx[fb].s);
        };
        Frag a0[2], a1[2], x0[4], x1[4];
        if (nstep > 0) {
            load_w(sl, 0, 0, a0);
            load_x(0, x0);
        }
        for (int s = 0; s < nstep; s += 2) {
            const int s1 = min(s + 1, nstep - 1), s2 = min(s + 2, nstep - 1);
            load_w(sl, s1 / ncs, s1 % ncs, a1);
            load_x(s1, x1);
            mma(a0, x0);
            if (s + 1 >= nstep) break;
            load_w(sl, s2 / ncs, s2 % ncs, a0);
            load_x(s2, x0);
            mma(a1, x1);
        }
    }
    if (idle) return;

    const int n_store = a.pool ? TILE - 1 : TILE;
    if (a.ksplit > 1) {
        // raw partial sums; channel of register g: (g & 3) + 8 (g >> 2) + 4h -> four consecutive channels per g >> 2
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const int col = fb * 32 + r, m = m0 + col;
                if (col >= n_store || m >= a.M) continue;
                float* dst = a.ws + ((size_t)ks * a.M + m) * a.n_out + gr.c_off + ch0 + cb * 32 + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(dst + 8 * q) =
                        float4{acc[cb][fb][4 * q], acc[cb][fb][4 * q + 1], acc[cb][fb][4 * q + 2], acc[cb][fb][4 * q + 3]};
            }
        return;
    }

#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int cbase = gr.c_off + ch0 + cb * 32;
        float sc[16], sh[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int ch = cbase + (g & 3) + 8 * (g >> 2) + 4 * h;
            sc[g] = a.scale[ch];
            sh[g] = a.shift[ch];
        }
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                float y = fmaf(acc[cb][fb][g], sc[g], sh[g]);
                if (a.act == VC_ACT_RELU) y = fmaxf(y, 0.0f);
                acc[cb][fb][g] = y;
            }
        if (a.pool) {
            // y[t] = max(y[t], y[t + 1]) inside a window; frame t + 1 is lane + 1, or lane 0 of the next 32-frame tile
            const int nxt_lane = (lane & 32) | ((lane + 1) & 31), first_lane = lane & 32;
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const int m = m0 + fb * 32 + r;
                const bool last = !live[fb] || tloc[fb] == a.T - 1;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float same = __shfl(acc[cb][fb][g], nxt_lane);
                    const float next = fb < 3 ? __shfl(acc[cb][fb < 3 ? fb + 1 : fb][g], first_lane) : 0.0f;
                    const float nb = r == 31 ? next : same;
                    if (!last && m + 1 < a.M) acc[cb][fb][g] = fmaxf(acc[cb][fb][g], nb);
                }
            }
        }
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const int col = fb * 32 + r, m = m0 + col;
            const bool st = col < n_store && m < a.M;
            if (a.out_mode == VC_MX8_OUT_MX) {
                float amax = 0.0f;
#pragma unroll
                for (int g = 0; g < 16; ++g) amax = fmaxf(amax, fabsf(acc[cb][fb][g]));
                amax = fmaxf(amax, __shfl_xor(amax, 32));
                if (!st) continue;
                const int e = amax > 0.0f ? vc::mx8_scale_exp(amax) : 0;
                uint8_t* dst = reinterpret_cast<uint8_t*>(a.C) + (size_t)m * a.n_out + cbase + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint32_t w = 0;
                    if (amax > 0.0f)
#pragma unroll
                        for (int i = 0; i < 4; ++i) w |= vc::mx8_encode(acc[cb][fb][4 * q + i], e) << (8 * i);
                    *reinterpret_cast<uint32_t*>(dst + 8 * q) = w;
                }
                if (h == 0) a.Cs[(size_t)m * (a.n_out >> 5) + (cbase >> 5)] = (uint8_t)(amax > 0.0f ? e + 127 : 0);
            } else if (st && a.out_mode == VC_MX8_OUT_BF16) {
                uint16_t* dst = reinterpret_cast<uint16_t*>(a.C) + (size_t)m * a.n_out + cbase + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<uint2*>(dst + 8 * q) =
                        uint2{bf16_rne(acc[cb][fb][4 * q]) | (bf16_rne(acc[cb][fb][4 * q + 1]) << 16),
                              bf16_rne(acc[cb][fb][4 * q + 2]) | (bf16_rne(acc[cb][fb][4 * q + 3]) << 16)};
            } else if (st) {
                float* dst = reinterpret_cast<float*>(a.C) + (size_t)m * a.n_out + cbase + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(dst + 8 * q) =
                        float4{acc[cb][fb][4 * q], acc[cb][fb][4 * q + 1], acc[cb][fb][4 * q + 2], acc[cb][fb][4 * q + 3]};
            }
        }
    }
}

// split K: sum the partial tiles in split order, then the epilogue (no pool); one thread per 4 channels
__global__ void __launch_bounds__(256)
mx8_reduce_kernel(const float* __restrict__ ws, int ksplit, int M, int n_out, const float* __restrict__ scale,
                  const float* __restrict__ shift, int act, int out_mode, void* C) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t total = (size_t)M * n_out;
    if (i >= total) return;
    float4 s = *reinterpret_cast<const float4*>(ws + i);
    for (int k = 1; k < ksplit; ++k) {
        const float4 p = *reinterpret_cast<const float4*>(ws + (size_t)k * total + i);
        s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    const int ch = (int)(i % n_out);
    float y[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        y[q] = fmaf(y[q], scale[ch + q], shift[ch + q]);
        if (act == VC_ACT_RELU) y[q] = fmaxf(y[q], 0.0f);
    }
    if (out_mode == VC_MX8_OUT_BF16)
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(C) + i) =
            uint2{bf16_rne(y[0]) | (bf16_rne(y[1]) << 16), bf16_rne(y[2]) | (bf16_rne(y[3]) << 16)};
    else
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(C) + i) = float4{y[0], y[1], y[2], y[3]};
}

// one thread per (row, 32-channel block)
template <typename TIn>
__global__ void __launch_bounds__(256)
mx8_quantize_kernel(const TIn* __restrict__ X, int M, int C, int ldx, uint8_t* __restrict__ Q, uint8_t* __restrict__ S) {
    const int nb = C >> 5;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)M * nb) return;
    const int m = (int)(id / nb), b = (int)(id % nb);
    const TIn* src = X + (size_t)m * ldx + 32 * b;
    float v[32];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        if constexpr (sizeof(TIn) == 2)
            v[i] = __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(src)[i] << 16);
        else
            v[i] = src[i];
        amax = fmaxf(amax, fabsf(v[i]));
    }
    const int e = amax > 0.0f ? vc::mx8_scale_exp(amax) : 0;
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        w[q] = 0;
        if (amax > 0.0f)
#pragma unroll
            for (int i = 0; i < 4; ++i) w[q] |= vc::mx8_encode(v[4 * q + i], e) << (8 * i);
    }
    uint4* dst = reinterpret_cast<uint4*>(Q + (size_t)m * C + 32 * b);
    dst[0] = uint4{w[0], w[1], w[2], w[3]};
    dst[1] = uint4{w[4], w[5], w[6], w[7]};
    S[(size_t)m * nb + b] = (uint8_t)(amax > 0.0f ? e + 127 : 0);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int mx8_ksplit(const vc_mx8_conv_desc* d) {
    if (d->pool || d->n_groups > 2 || d->out_mode == VC_MX8_OUT_MX || d->M <= 0 || d->Cin < 64) return 1;
    const int tiles = (d->M + TILE - 1) / TILE;
    const int nslab = d->Cin / slab_of(d->Cin);
    int k = std::min(MAX_SPLIT, (800 + tiles - 1) / tiles);
    k = std::min(k, nslab);
    return k > 1 ? k : 1;
}

}  // namespace

extern "C" {

int vc_mx8_quantize(const void* d_X, int32_t x_dtype, int32_t M, int32_t C, int32_t ldx, void* d_Q, void* d_S, void* stream) {
    VC_REQUIRE(d_X && d_Q && d_S, "vc_mx8_quantize: NULL argument");
    VC_REQUIRE(x_dtype == VC_F32 || x_dtype == VC_BF16, "vc_mx8_quantize: x_dtype must be VC_F32 or VC_BF16");
    VC_REQUIRE(M > 0 && C >= 32 && (C & 31) == 0 && ldx >= C, "vc_mx8_quantize: bad shape M=%d C=%d ldx=%d", M, C, ldx);
    VC_REQUIRE(aligned16(d_Q), "vc_mx8_quantize: d_Q must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)M * (C >> 5);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (x_dtype == VC_F32)
        hipLaunchKernelGGL(mx8_quantize_kernel<float>, dim3(blocks), dim3(256), 0, st, static_cast<const float*>(d_X), M, C,
                           ldx, static_cast<uint8_t*>(d_Q), static_cast<uint8_t*>(d_S));
    else
        hipLaunchKernelGGL(mx8_quantize_kernel<uint16_t>, dim3(blocks), dim3(256), 0, st, static_cast<const uint16_t*>(d_X),
                           M, C, ldx, static_cast<uint8_t*>(d_Q), static_cast<uint8_t*>(d_S));
    VC_HIP_CHECK(hipGetLastError());
    return VC_OK;
}

size_t vc_mx8_conv_workspace_bytes(const vc_mx8_conv_desc* d) {
    if (!d) return 0;
    const int k = mx8_ksplit(d);
    return k > 1 ? (size_t)k * d->M * d->n_out * sizeof(float) : 0;
}

int vc_mx8_conv(const vc_mx8_conv_desc* d, void* stream) {
    VC_REQUIRE(d && d->d_X && d->d_Xs && d->d_C && d->d_epi_scale && d->d_epi_shift, "vc_mx8_conv: NULL argument");
    VC_REQUIRE(d->M > 0 && d->T > 0 && d->M % d->T == 0 && d->Cin >= 64 && (d->Cin & 63) == 0,
               "vc_mx8_conv: bad shape M=%d T=%d Cin=%d", d->M, d->T, d->Cin);
    VC_REQUIRE(d->n_groups >= 1 && d->n_groups <= VC_MX8_MAX_GROUPS && d->n_out >= 32 && (d->n_out & 31) == 0,
               "vc_mx8_conv: bad group count %d / n_out %d", d->n_groups, d->n_out);
    VC_REQUIRE(d->out_mode >= VC_MX8_OUT_MX && d->out_mode <= VC_MX8_OUT_F32, "vc_mx8_conv: bad out_mode %d", d->out_mode);
    VC_REQUIRE(d->act == VC_ACT_NONE || d->act == VC_ACT_RELU, "vc_mx8_conv: act must be none or relu");
    VC_REQUIRE(d->out_mode != VC_MX8_OUT_MX || d->d_Cs, "vc_mx8_conv: MX output needs d_Cs");
    VC_REQUIRE(aligned16(d->d_X) && aligned16(d->d_C), "vc_mx8_conv: d_X / d_C must be 16-byte aligned");
    for (int i = 0; i < d->n_groups; ++i) {
        const vc_mx8_group& g = d->groups[i];
        VC_REQUIRE(g.d_W && g.d_Ws && aligned16(g.d_W), "vc_mx8_conv: group %d: NULL or unaligned weights", i);
        VC_REQUIRE(g.taps >= 1 && g.taps <= 32 && g.pad_l >= 0 && g.pad_l < g.taps && g.c_off >= 0 && (g.c_off & 31) == 0 &&
                   g.c_off + 128 <= d->n_out, "vc_mx8_conv: group %d: bad taps %d / pad_l %d / c_off %d", i, g.taps, g.pad_l, g.c_off);
        if (i & 1)
            VC_REQUIRE(g.pad_l == d->groups[i - 1].pad_l, "vc_mx8_conv: groups %d and %d must share pad_l", i - 1, i);
    }
    Mx8Args a{};
    a.X = static_cast<const uint8_t*>(d->d_X);
    a.Xs = static_cast<const uint8_t*>(d->d_Xs);
    a.M = d->M; a.T = d->T; a.Cin = d->Cin; a.n_groups = d->n_groups;
    for (int i = 0; i < d->n_groups; ++i) a.g[i] = d->groups[i];
    a.scale = d->d_epi_scale; a.shift = d->d_epi_shift;
    a.act = d->act; a.pool = d->pool ? 1 : 0; a.out_mode = d->out_mode; a.n_out = d->n_out;
    a.C = d->d_C; a.Cs = static_cast<uint8_t*>(d->d_Cs);
    a.ksplit = 1;
    const int k = mx8_ksplit(d);
    if (k > 1 && d->d_workspace && d->workspace_bytes >= vc_mx8_conv_workspace_bytes(d)) {
        for (int i = 1; i < d->n_groups; ++i)
            VC_REQUIRE(d->groups[i].taps == d->groups[0].taps, "vc_mx8_conv: split K needs equal taps");
        VC_REQUIRE(aligned16(d->d_workspace), "vc_mx8_conv: unaligned workspace");
        a.ksplit = k;
        a.ws = static_cast<float*>(d->d_workspace);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int step = a.pool ? TILE - 1 : TILE;
    dim3 grid((d->M + step - 1) / step, (d->n_groups + 1) / 2, a.ksplit);
    int max_taps = 1;
    for (int i = 0; i < d->n_groups; ++i) max_taps = std::max(max_taps, d->groups[i].taps);
    hipLaunchKernelGGL(mx8_conv_kernel, grid, dim3(NT), lds_bytes(d->Cin, max_taps), st, a);
    VC_HIP_CHECK(hipGetLastError());
    if (a.ksplit > 1) {
        const size_t n4 = (size_t)d->M * d->n_out / 4;
        hipLaunchKernelGGL(mx8_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a.ws, a.ksplit, d->M,
                           d->n_out, d->d_epi_scale, d->d_epi_shift, d->act, d->out_mode, d->d_C);
        VC_HIP_CHECK(hipGetLastError());
    }
    return VC_OK;
}

}  // extern "C"
