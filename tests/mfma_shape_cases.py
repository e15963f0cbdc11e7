"""Cases for the 16x16x32 fragment and accumulator maps of the bank, projection and conv256 tile kernels: what the shapes of
tests/conv_gemm_cases.py do not reach.  Same integer grid (make_exact), so the device must equal float64 exactly;
tests/test_mfma_shape_cpu.py proves that and that every case lands on its kernel form, tests/test_mfma_shape_gpu.py runs
them."""
import numpy as np

import conv_gemm_ref as R
from conv_gemm_cases import case
from conv_gemm_ref import ACT_NONE, ACT_RELU, BF16


def _bank_pads(K):
    return tuple((k - 1) // 2 if k % 2 else (k - 2) // 2 for k in range(1, K + 1))


# two windows of 130 frames: two row tiles (the second holds 4 real frames and 252 clamped rows), the window edge at frame
# 130 = 8 * 16 + 2 inside a 16-frame fragment tile
M2, T2 = 260, 130

# every tap 0..31 (every tap offset mod 8 of the swizzle) in one launch
BANK_TAPS = case('shape_bank_K32', 'bank256', BF16, M2, T2, 64, 128, tuple(range(1, 33)), pad_l=_bank_pads(32), act=ACT_RELU,
                 ldc=128 * 32 + 8, ldx=72, toggle=('bank256',))
# two slabs = four k = 32 steps with a switch of the resident activation buffer; stored plain and max-pooled
BANK_CIN128 = [case('shape_bank_cin128_pool%d' % pool, 'bank256', BF16, M2, T2, 128, 128, (1, 2, 3, 4), pad_l=_bank_pads(4), act=ACT_RELU,
                    epi_pool=pool, ldc=520, ldx=136, toggle=() if pool else ('bank256',)) for pool in (0, 1)]

# K split over two workgroups per row tile.  The library gives a projection to the bank tiles from M >= 1024 and
# taps * Cin >= 4096 on (proj256_ok, csrc/vc_gemm.hip), so eight slabs -- the least the split accepts -- need 8 taps, and
# k = 3 needs 22 slabs; M = 4 x 257 leaves 4 real frames in the fifth row tile.
PROJ_SPLIT = [case('shape_proj_split_cin512_k8', 'proj256', BF16, 1028, 257, 512, 256, (8,), ws='full', c_off=(8,), ldc=272, ldx=520,
                   toggle=('proj256', 'proj256_split')),
              case('shape_proj_split_cin1408_k3', 'proj256', BF16, 1028, 257, 1408, 256, (3,), ws='full', act=ACT_RELU, c_off=(8,), ldc=272,
                   ldx=1416, toggle=('proj256', 'proj256_split'))]

# conv256: k = 3 over two slabs, three windows of 100 frames (300 = two 128-row blocks and 44 rows of a third), with and
# without the operand pool; and the same projection at eight slabs and 256 columns (the 8-wave block)
CONV256 = [case('shape_conv256_pool%d' % pool, 'conv256', BF16, 300, 100, 128, 128, (3,), pro_pool=pool, act=ACT_RELU, ldc=136, ldx=136,
                toggle=('conv256',)) for pool in (0, 2)] + \
          [case('shape_conv256_cin512_N256', 'conv256', BF16, 300, 100, 512, 256, (3,), ldc=264, ldx=520, toggle=('conv256',))]

EXACT = [BANK_TAPS] + BANK_CIN128 + PROJ_SPLIT + CONV256


def signed_zero_pool(s, d):
    """In the pooled operand of `d` (values >= 0), frames 3 and 50 of every window become -0.0 where the next frame is
    positive, and frame 99 (the window's last, which pools with itself) becomes -0.0 everywhere."""
    assert s.pro_pool == 2 and s.T == 100
    X = d.X.reshape(s.M // s.T, s.T, -1)
    for t in (3, 50):
        X[:, t] = np.where(X[:, t + 1] > 0, -0.0, X[:, t])
    X[:, 99] = -0.0
    return d


# ---- one-hot placement: the bank of widths 1..4 on one 64-channel slab, two windows of 130 frames
ONE_HOT = case('shape_bank_one_hot', 'bank256', BF16, M2, T2, 64, 128, (1, 2, 3, 4), pad_l=_bank_pads(4), epi_scale=0, epi_shift=0, ldc=520,
               ldx=72)
# (frame, channel) of the single 1.0: frames 15 | 16 of a fragment's row tile, channels 31 | 32 (the two k = 32 steps of a
# slab); frame 17 sends the wider filter's extra tap (tap 3 of width 4, pad_l 1) to output frame 15, frames 129 | 130 sit on
# either side of the window edge
ONE_HOT_AT = [(15, 5), (16, 5), (40, 31), (40, 32), (17, 63), (129, 7), (130, 0)]


def weight_code(g, oc, j, ch):
    """A small integer (bf16 holds it) that differs between neighbouring output channels, taps and channels."""
    return (oc * 37 + j * 11 + ch * 3 + g * 5) % 253 - 126


def make_one_hot(frame, ch):
    s = ONE_HOT
    X = np.zeros((s.M, s.Cin))
    X[frame, ch] = 1.0
    oc, cc = np.arange(s.N)[:, None, None], np.arange(s.Cin)[None, None, :]
    groups = []
    for g, taps in enumerate(s.taps):
        W = weight_code(g, oc, np.arange(taps)[None, :, None], cc).reshape(s.N, taps * s.Cin)
        groups.append(R.group(W, taps, s.pad_l[g], s.c_off[g]))
    return R.desc(X, s.T, s.N, groups, dtype=BF16, Cin=s.Cin, act=ACT_NONE, ldc=s.ldc)
