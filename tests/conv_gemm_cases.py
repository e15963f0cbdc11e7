"""The cases tests/test_conv_gemm_gpu.py runs on the device and tests/test_conv_gemm_cpu.py proves sound without one: the
table of EXACT cases (one row per launch, grouped by the kernel form launch() of csrc/vc_gemm.hip selects), launch()'s
conditions restated on the host (expected_form), the integer-grid operands of a case (make_exact), and exactness(),
which bounds every intermediate of a case so that float32 arithmetic is exact in any summation order."""
import types
import zlib

import numpy as np

import conv_gemm_ref as R
from conv_gemm_ref import ACT_NONE, ACT_RELU, BF16, F32, HIGHWAY, PLAIN

CONV_MAX_TAPS = 32


# ------------------------------------------------------------------------------------------ the case table
def case(name, form, dtype, M, T, Cin, N, taps=(1,), **kw):
    """One launch.  taps: per group; pad_l defaults to (taps - 1) // 2, c_off to the concat layout g * N."""
    s = types.SimpleNamespace(name=name, form=form, dtype=dtype, M=M, T=T, Cin=Cin, N=N, taps=tuple(taps), mode=PLAIN,
                              pad_l=None, c_off=None, ldx=None, ldc=None, ldr=0, pro_affine=0, pro_relu=0, pro_pool=0,
                              epi_scale=1, epi_shift=1, act=ACT_NONE, out_f32=0, drop_keep=0.0, drop_seed=0, sum_groups=0,
                              epi_pool=0, toggle=(), ws=None, hw_half=1, density=None, variant=None)
    for k, v in kw.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    n = len(s.taps)
    if s.pad_l is None:
        s.pad_l = tuple((t - 1) // 2 for t in s.taps)
    if s.c_off is None:
        s.c_off = tuple(g * Cin for g in range(n)) if s.sum_groups else tuple(g * N for g in range(n))
    vec = 4 if dtype == F32 else 8
    xw = (max(s.c_off) + Cin) if s.sum_groups else Cin
    if s.ldx is None:
        s.ldx = xw + vec                                   # ldx > Cin everywhere: the padding columns hold NaN
    if s.ldc is None:
        s.ldc = (Cin if s.mode == HIGHWAY else N if s.sum_groups else max(s.c_off) + N) + 5
    assert M % T == 0 and s.ldx % vec == 0 and s.ldx >= xw, name
    return s


def _pro(i):
    """The prologue variants in rotation: PRO 0, PRO 1 (pool, either order), PRO 2 with every combination the training
    path and the header allow."""
    return [dict(), dict(pro_pool=1), dict(pro_pool=2), dict(pro_affine=1), dict(pro_affine=1, pro_relu=1, pro_pool=1),
            dict(pro_relu=1, pro_pool=2), dict(pro_affine=1, pro_pool=1), dict(pro_affine=1, pro_pool=2)][i % 8]


def _epi(i):
    return [dict(), dict(epi_scale=0), dict(epi_shift=0), dict(act=ACT_RELU), dict(epi_scale=0, epi_shift=0)][i % 5]


def _cases():
    out = []
    Ms, Ns = (1, 63, 64, 65, 127, 128, 129), (1, 31, 32, 33, 127, 128, 129)
    for dt, dn, slab in ((F32, 'f32', 32), (BF16, 'bf16', 64)):
        # ---- gemm_kernel MI = 1, taps = 1 (dense): every M x N tile edge; K = Cin in {8, 40}, never a whole slab
        i = 0
        for M in Ms:
            for N in Ns:
                i += 1
                kw = dict(_epi(i))
                c0 = (0, 3, 8, 0)[i % 4]                  # 3: (c_off * element size) % 16 != 0 -> the scalar store path
                kw.update(c_off=(c0,), ldc=c0 + N + (5, 8 - (c0 + N) % 8, 3)[i % 3], out_f32=i % 2)
                if i % 3 == 0:
                    kw.update(ldr=N + 3)
                if i % 7 == 0:
                    kw.update(_pro(3 + i % 5))
                out.append(case('dense_%s_M%d_N%d' % (dn, M, N), 'gemm_mi1', dt, M, (1 if M % 2 else M // 2) if i % 2 else M,
                                (8, 40)[i % 2], N, **kw))
        # ---- gemm_kernel MI = 1, taps > 1 (Toeplitz path)
        i = 0
        for taps in (2, 3, 4, 5, 8, 33):
            for T in sorted({1, 2, taps - 1, 37}):
                i += 1
                nw = (3, 2, 5)[i % 3]
                kw = dict(_pro(i)); kw.update(_epi(i))
                kw.update(out_f32=i % 2, ldr=(0, (1, 33, 129)[i % 3] + 4)[i % 2])
                if i % 4 == 0:
                    kw.update(pad_l=((0, taps - 1)[(i // 4) % 2],))
                out.append(case('toep_%s_k%d_T%d' % (dn, taps, T), 'gemm_mi1', dt, T * nw, T, (8, 40)[i % 2], (1, 33, 129)[i % 3],
                                (taps,), **kw))
        # M >= 128 but Cin no whole slab; and taps past CONV_MAX_TAPS with a whole slab
        out.append(case('toep_%s_M148_cin40' % dn, 'gemm_mi1', dt, 148, 37, 40, 33, (3,), pro_affine=1, pro_relu=1, ldr=36, out_f32=1))
        out.append(case('toep_%s_M148_k33' % dn, 'gemm_mi1', dt, 148, 37, slab, 31, (33,), pro_pool=1, out_f32=1))
        out.append(case('toep_%s_groups' % dn, 'gemm_mi1', dt, 74, 37, 40, 31, (1, 2, 5), c_off=(0, 35, 70), ldc=104, act=ACT_RELU, out_f32=1))
        # ---- gemm_kernel MI = 2: >= 512 blocks of 128 rows
        out.append(case('mi2_%s_65536x8x100' % dn, 'gemm_mi2', dt, 65536, 64, 8, 100, act=ACT_RELU, out_f32=1, ldr=104))
        out.append(case('mi2_%s_32groups' % dn, 'gemm_mi2', dt, 2048, 128, 8, 128, (1,) * 32, ldc=4096, out_f32=1))
        out.append(case('mi2_%s_toeplitz_affine' % dn, 'gemm_mi2', dt, 65536, 16, 8, 20, (3,), pro_affine=1, pro_relu=1, pro_pool=1, out_f32=1))
        # ---- highway mode
        i = 0
        for H in (8, 24, 32, 40, 72, 128):
            for M in (1, 65, 129):
                i += 1
                o32 = i % 2
                out.append(case('highway_%s_H%d_M%d' % (dn, H, M), 'highway_mi1', dt, M, M, H, 64 * ((H + 31) // 32), mode=HIGHWAY,
                                ldc=H + 8, out_f32=o32, hw_half=1 if (o32 or dt == F32) else 0, epi_scale=0))
        # ---- conv_kernel: taps in [2, 32], Cin a whole number of slabs, M >= 128
        i = 0
        for M, T in ((128, 128), (128, 64), (128, 1), (128, 2), (129, 43), (129, 129), (129, 3), (255, 85), (255, 5), (255, 255),
                     (256, 256), (256, 32)):
            for taps in ((2, 7, 32)[i % 3], (2, 7, 32)[(i + 1) % 3]):
                i += 1
                N = (1, 129)[i % 2]
                kw = dict(_pro(i)); kw.update(_epi(i + 2))
                kw.update(out_f32=(i // 2) % 2, ldr=(0, N + 2)[i % 2], c_off=((0, 3, 129)[i % 3],))
                out.append(case('conv_%s_M%d_T%d_k%d' % (dn, M, T, taps), 'conv_kernel', dt, M, T, slab * (1 + i % 2), N, (taps,), **kw))
        for j, pro in enumerate((dict(), dict(pro_pool=1), dict(pro_affine=1, pro_relu=1, pro_pool=1))):
            # groups with distinct taps and a taps = 1 member; c_off = 129 g breaks the 16-byte alignment of the stores
            out.append(case('conv_%s_groups_pro%d' % (dn, j), 'conv_kernel', dt, 129, 43, slab, 129, (1, 2, 7, 4), out_f32=j % 2,
                            pad_l=(0, 1, 3, 0), act=ACT_RELU, **pro))
        # ---- conv_kernel, sum_groups: 1 and S > 1
        out.append(case('sum1_%s_3groups' % dn, 'conv_kernel', dt, 256, 64, slab, 40, (1, 2, 3), sum_groups=1, out_f32=1, ldr=44, act=ACT_RELU))
        out.append(case('sum1_%s_4groups_pro' % dn, 'conv_kernel', dt, 129, 43, slab, 129, (1, 2, 3, 4), sum_groups=1, out_f32=1,
                        pro_affine=1, pro_relu=1, pro_pool=1))
        out.append(case('sum1_%s_stored' % dn, 'conv_kernel', dt, 128, 32, slab, 33, (2, 5), sum_groups=1, pro_pool=2, ldr=36))
        for n, S in ((3, 2), (4, 2), (5, 3), (8, 4)):
            out.append(case('sumS_%s_n%d_S%d' % (dn, n, S), 'conv_kernel', dt, 256, 64, slab, (40, 129)[n % 2], tuple(range(1, n + 1)),
                            sum_groups=S, out_f32=1, epi_scale=0, epi_shift=0))
    dt, dn = BF16, 'bf16'
    # ---- vc_conv256 (bf16): N % 128 == 0, Cin % 64 == 0, M >= 128, taps <= 7, K >= 384, plain or pro_pool = 2 operand
    i = 0
    for M, T in ((128, 64), (129, 43), (2047, 89), (2048, 256)):
        for taps, Cin in ((1, 384), (2, 192), (7, 64)):
            i += 1
            N = (128, 256)[i % 2] if M < 2047 else (128, 128, 256)[i % 3]
            kw = dict(_epi(i))
            out.append(case('conv256_M%d_k%d_N%d' % (M, taps, N), 'conv256', dt, M, T, Cin, N, (taps,), pro_pool=(0, 2)[i % 2],
                            ldr=(0, N + 4)[(i // 2) % 2], c_off=((0, 8)[i % 2],), ldc=N + 16, ldx=Cin + 8, toggle=('conv256',), **kw))
    # ---- vc_bank256 (bf16): pairs of 128-filter groups (2p+1, 2p+2) taps wide, M >= 256
    i = 0
    for M, T in ((256, 256), (256, 1), (257, 1), (257, 257), (511, 73), (510, 255)):
        for K in ((2, 4, 32)[i % 3], (2, 4, 32)[(i + 1) % 3]):
            i += 1
            if K == 32 and M > 257:
                K = 4
            pool = i % 2
            out.append(case('bank256_M%d_T%d_K%d_pool%d' % (M, T, K, pool), 'bank256', dt, M, T, (64, 128)[(i // 2) % 2], 128,
                            tuple(range(1, K + 1)), pad_l=tuple((k - 1) // 2 if k % 2 else (k - 2) // 2 for k in range(1, K + 1)),
                            epi_pool=pool, act=ACT_RELU if pool else (ACT_NONE, ACT_RELU)[(i // 2) % 2],
                            ldc=128 * K + 8, ldx=(64, 128)[(i // 2) % 2] + 8, toggle=() if pool else ('bank256',)))
    # ---- proj256 (bf16): N = 256, M >= 1024, taps in [2, 32], K >= 4096; K split in two when Cin / 64 >= 8
    for M, T in ((1024, 256), (1025, 205)):
        for taps, Cin in ((2, 2048), (32, 128)):
            for ws in ('full', 'none', 'small', 'misaligned'):
                if ws != 'full' and (Cin == 128 or M == 1024):
                    continue                                  # the workspace only matters where K is split
                out.append(case('proj256_M%d_k%d_%s' % (M, taps, ws), 'proj256', dt, M, T, Cin, 256, (taps,), ws=ws if Cin == 2048 else None,
                                act=(ACT_NONE, ACT_RELU)[taps == 32], c_off=(8,), ldc=272, ldx=Cin + 8,
                                toggle=('proj256', 'proj256_split') if ws == 'full' else ()))
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return out


def _isolation_cases():
    """Three windows each (tests/test_conv_gemm_gpu.py poisons the middle one): taps > 1, operand pool, pooled epilogue."""
    out = []
    for dt, dn, slab in ((F32, 'f32', 32), (BF16, 'bf16', 64)):
        out += [case('iso_gemm_%s_pool' % dn, 'gemm_mi1', dt, 60, 20, 8, 33, (3,), pro_pool=1, out_f32=1),
                case('iso_gemm_%s_pro2' % dn, 'gemm_mi1', dt, 60, 20, 40, 33, (5,), pro_affine=1, pro_relu=1, pro_pool=1, out_f32=1),
                case('iso_conv_%s_pool' % dn, 'conv_kernel', dt, 150, 50, slab, 33, (7,), pro_pool=1, out_f32=1),
                case('iso_conv_%s_pro2' % dn, 'conv_kernel', dt, 150, 50, slab, 129, (2,), pro_affine=1, pro_relu=1, pro_pool=1, ldr=132),
                case('iso_sum_%s' % dn, 'conv_kernel', dt, 150, 50, slab, 33, (1, 2, 3), sum_groups=1, pro_pool=2, out_f32=1),
                # gemm_kernel MI = 2: 513 blocks of 128 rows, three windows of 21,846 frames
                case('iso_mi2_%s_pro2' % dn, 'gemm_mi2', dt, 3 * 21846, 21846, 8, 20, (3,), pro_affine=1, pro_relu=1, pro_pool=1,
                     out_f32=1)]
    out += [case('iso_conv256_pool', 'conv256', BF16, 192, 64, 64, 128, (7,), pro_pool=2, ldc=136, ldx=72, ldr=132),
            case('iso_conv256_wide', 'conv256', BF16, 192, 64, 192, 256, (2,), ldc=264, ldx=200),
            case('iso_bank256', 'bank256', BF16, 300, 100, 64, 128, (1, 2, 3, 4), pad_l=(0, 0, 1, 1), ldc=520, ldx=72, act=ACT_RELU),
            case('iso_bank256_epi_pool', 'bank256', BF16, 300, 100, 64, 128, (1, 2, 3, 4), pad_l=(0, 0, 1, 1), ldc=520, ldx=72,
                 act=ACT_RELU, epi_pool=1),
            case('iso_bank256_epi_pool_tile_edge', 'bank256', BF16, 765, 255, 64, 128, (1, 2), pad_l=(0, 0), ldc=264, ldx=72,
                 act=ACT_RELU, epi_pool=1),
            case('iso_proj256_split', 'proj256', BF16, 1026, 342, 2048, 256, (2,), ldc=264, ldx=2056, ws='full'),
            case('iso_proj256', 'proj256', BF16, 1026, 342, 128, 256, (32,), ldc=264, ldx=136, act=ACT_RELU)]
    return out


def _dn(dt):
    return ('f32', 'bf16')[dt]


def _order_cases():
    """Prologue order: a shifting affine prologue without ReLU in front of taps > 1, pool off and on (make_order)."""
    return [case('order_%s_%s_pool%d' % (form, _dn(dt), pool), form, dt, M, T, Cin, 3, (taps,), pro_affine=1, pro_pool=pool, out_f32=1)
            for form, dt, M, T, Cin, taps in (('gemm_mi1', F32, 20, 5, 8, 4), ('gemm_mi1', BF16, 20, 5, 8, 4),
                                              ('conv_kernel', F32, 129, 43, 32, 7), ('conv_kernel', BF16, 129, 43, 64, 7))
            for pool in (0, 1)]


def make_order(s):
    """X = 0, pro_scale = 1, pro_shift = 1, all-ones weights: every real frame contributes Cin, every padding frame 0."""
    taps = s.taps[0]
    return R.desc(np.zeros((s.M, s.Cin)), s.T, s.N, [R.group(np.ones((s.N, taps * s.Cin)), taps, s.pad_l[0], 0)], dtype=s.dtype,
                  pro_scale=np.ones(s.Cin), pro_shift=np.ones(s.Cin), pro_pool=s.pro_pool, ldc=s.ldc, out_f32=1)


_ZERO_VARIANTS = dict(pool2=dict(pro_pool=2), relu_pool1=dict(pro_relu=1, pro_pool=1),
                      scale_to_minus_zero=dict(pro_affine=1, pro_relu=1, pro_pool=1))


def _zero_cases():
    """Signed zeros through the non-negative pool (vc_conv256 takes no affine / relu prologue: conv256_ok)."""
    rows = [(f, dt, M, T, Cin, N, v) for f, dt, M, T, Cin, N in (('gemm_mi1', F32, 24, 6, 8, 5), ('gemm_mi1', BF16, 24, 6, 8, 5),
                                                                 ('conv_kernel', F32, 132, 6, 32, 5), ('conv_kernel', BF16, 132, 6, 64, 5))
            for v in ('pool2', 'relu_pool1', 'scale_to_minus_zero')] + [('conv256', BF16, 132, 6, 192, 128, 'pool2')]
    return [case('zeros_%s_%s_%s' % (f, _dn(dt), v), f, dt, M, T, Cin, N, (2,), pad_l=(0,), ldc=N + 8, ldx=Cin + 8,
                 out_f32=0 if f == 'conv256' else 1, variant=v, **_ZERO_VARIANTS[v]) for f, dt, M, T, Cin, N, v in rows]


def make_zeros(s):
    """-0.0, +0.0 and positive frames: every pattern meets every other as (x[t], x[t+1]) and at the window's end."""
    rng = np.random.RandomState(7)
    M, T, Cin, N = s.M, s.T, s.Cin, s.N
    pat = np.array([-0.0, 1.0, -0.0, 0.0, 2.0, -0.0])
    assert T == len(pat)
    X = np.repeat(np.tile(pat, M // T)[:, None], Cin, 1)
    X[:, 1::2] = np.repeat(np.tile(pat[::-1], M // T)[:, None], Cin // 2, 1)
    scale = shift = None
    if s.variant == 'scale_to_minus_zero':
        X = -X                                                             # +0.0 * -1 + -0.0 = -0.0; the positives come back
        scale, shift = -np.ones(Cin), np.where(np.arange(Cin) % 4 < 2, -0.0, 0.0)
    W = rng.randint(-2, 3, (N, 2 * Cin)) * (rng.rand(N, 2 * Cin) < min(1.0, 20.0 / Cin))
    return R.desc(X, T, N, [R.group(W, 2, 0, 0)], dtype=s.dtype, pro_scale=scale, pro_shift=shift, pro_relu=s.pro_relu,
                  pro_pool=s.pro_pool, ldc=s.ldc, out_f32=s.out_f32)


DROP_C_OFF = 3


def _dropout_cases():
    """ldc > N and c_off > 0: the mask index is m * ldc + c_off + n.  ReLU on the integer grid with a residual."""
    return [case('drop_%s_%s_keep%g' % (form, _dn(dt), keep), form, dt, M, T, Cin, N, (taps,), c_off=(DROP_C_OFF,),
                 ldc=DROP_C_OFF + N + 6, out_f32=1, drop_keep=keep, drop_seed=0x1234567 + int(keep * 100), act=ACT_RELU, ldr=N + 1)
            for form, dt, M, T, Cin, N, taps in (('gemm_mi1', F32, 65, 65, 8, 33, 1), ('gemm_mi1', BF16, 65, 65, 8, 33, 1),
                                                 ('conv_kernel', F32, 129, 43, 32, 33, 2))
            for keep in (0.25, 0.9, 1.0)]


EXACT_CASES = _cases()
ISOLATION_CASES = _isolation_cases()
ORDER_CASES = _order_cases()
ZERO_CASES = _zero_cases()
DROPOUT_CASES = _dropout_cases()
FORMS = ('gemm_mi1', 'gemm_mi2', 'highway_mi1', 'conv_kernel', 'conv256', 'bank256', 'proj256')


def cases_of(form, dtype=None):
    return [s for s in EXACT_CASES if s.form == form and (dtype is None or s.dtype == dtype)]


# ------------------------------------------------------------------------------------------ launch() on the host
def _aligned(s):
    return s.ldx % 8 == 0 and s.ldc % 8 == 0 and all(c % 8 == 0 for c in s.c_off)


def _plain_epi(s):
    return not (s.pro_affine or s.pro_relu or s.ldr or s.out_f32 or s.drop_keep > 0.0)


def bank256_ok(s, opts):
    n = len(s.taps)
    if opts.get('bank256', -1) == 0 or s.dtype != BF16 or s.mode != PLAIN:
        return False
    if n < 2 or n % 2 or n > 32 or s.N != 128 or s.Cin % 64 or s.M < 256:
        return False
    if not _plain_epi(s) or s.pro_pool or s.act not in (ACT_NONE, ACT_RELU) or not _aligned(s):
        return False
    return all(s.taps[g + 1] == s.taps[g] + 1 and s.pad_l[g] == s.pad_l[g + 1] and s.taps[g + 1] <= 32 for g in range(0, n, 2))


def conv256_ok(s, opts):
    if opts.get('conv256', -1) == 0 or s.dtype != BF16 or s.mode != PLAIN or len(s.taps) != 1:
        return False
    if s.N % 128 or s.Cin % 64 or s.M < 128 or s.taps[0] > 7 or s.taps[0] * s.Cin < 384:
        return False
    if s.pro_affine or s.pro_relu or s.pro_pool == 1 or s.out_f32 or s.drop_keep > 0.0 or not _aligned(s):
        return False
    return not (s.ldr and s.ldr % 4)


def proj256_ok(s, opts):
    if opts.get('proj256', -1) == 0 or s.dtype != BF16 or s.mode != PLAIN or len(s.taps) != 1:
        return False
    if s.N != 256 or s.Cin % 64 or s.M < 1024 or not 2 <= s.taps[0] <= 32 or s.taps[0] * s.Cin < 4096:
        return False
    return _plain_epi(s) and not s.pro_pool and not s.epi_pool and s.act in (ACT_NONE, ACT_RELU) and _aligned(s)


def expected_form(s, opts=None):
    """launch() of csrc/vc_gemm.hip restated (16-byte aligned C assumed): which kernel form a case takes."""
    opts = opts or {}
    slab = 32 if s.dtype == F32 else 64
    if s.sum_groups:
        return 'conv_kernel'
    if proj256_ok(s, opts):
        return 'proj256'
    if conv256_ok(s, opts):
        return 'conv256'
    conv_ok = s.mode == PLAIN and s.Cin % slab == 0 and s.M >= 128 and max(s.taps) <= CONV_MAX_TAPS
    if conv_ok and max(s.taps) > 1:
        return 'bank256' if bank256_ok(s, opts) else 'conv_kernel'
    blocks128 = ((s.M + 127) // 128) * ((s.N + 127) // 128) * len(s.taps)
    return ('highway' if s.mode == HIGHWAY else 'gemm') + ('_mi1' if blocks128 < 512 else '_mi2')


# ------------------------------------------------------------------------------------------ integer-grid operands
def make_exact(s):
    """The reference descriptor of case `s` with its integer-grid operands (a pure function of the case's name)."""
    rng = np.random.RandomState(zlib.crc32(s.name.encode()) & 0x7FFFFFFF)
    n = len(s.taps)
    stored16 = s.dtype == BF16 and not s.out_f32
    nonneg = s.pro_pool == 2 and not s.pro_relu            # pro_pool = 2 promises pooled values >= 0
    xw = (max(s.c_off) + s.Cin) if s.sum_groups else s.Cin
    X = rng.randint(0 if nonneg else -3, 4, (s.M, xw)).astype(np.float64)
    pro_scale = pro_shift = None
    if s.pro_affine:
        pro_scale = rng.choice([1.0, 2.0] if nonneg else [1.0, 2.0, -1.0], s.Cin)
        pro_shift = rng.randint(0 if nonneg else -1, 2, s.Cin).astype(np.float64)
        pro_shift[pro_shift == 0] = 1.0                    # never zero: padding that took the shift would show
    if s.mode == HIGHWAY:
        H = s.Cin
        dens = 1.0 if not stored16 else min(1.0, 12.0 / H)
        W1 = rng.randint(-2, 3, (H, H)) * (rng.rand(H, H) < dens)
        W2 = rng.randint(-2, 3, (H, H)).astype(np.float64)
        b1 = rng.randint(1, 4, H) * rng.choice([-1, 1], H)
        cls = np.arange(H) % (3 if s.hw_half else 2)       # gate saturated open / closed / exactly one half
        W2[:, cls == 2] = 0.0
        b2 = np.where(cls == 0, 2048.0, np.where(cls == 1, -2048.0, 0.0))
        Bt, sh = R.highway_pack(W1, b1, W2, b2)
        return R.desc(X, s.T, s.N, [R.group(Bt, 1, 0, 0)], dtype=s.dtype, mode=HIGHWAY, epi_shift=sh, ldc=s.ldc, out_f32=s.out_f32)
    ktot = sum(t * s.Cin for t in s.taps) if s.sum_groups else None
    groups = []
    for g in range(n):
        K = s.taps[g] * s.Cin
        dens = 1.0
        if stored16:
            dens = s.density if s.density else min(1.0, (8.0 if s.pro_affine else 25.0) / (ktot or K))
        W = rng.randint(-2, 3, (s.N, K)) * (rng.rand(s.N, K) < dens)
        groups.append(R.group(W, s.taps[g], s.pad_l[g], s.c_off[g]))
    width = s.N if s.sum_groups else max(s.c_off) + s.N
    epi_scale = rng.choice([1.0, -1.0, 2.0] if stored16 else [0.5, 1.0, 2.0, -1.0], width) if s.epi_scale else None
    epi_shift = None
    if s.epi_shift:
        epi_shift = rng.randint(-2, 3, width).astype(np.float64)
        epi_shift[epi_shift == 0] = 1.0                    # a shift taken from the wrong column changes an integer
    Rr = rng.randint(-3, 4, (s.M, s.N)).astype(np.float64) if s.ldr else None
    return R.desc(X, s.T, s.N, groups, dtype=s.dtype, Cin=s.Cin, pro_scale=pro_scale, pro_shift=pro_shift, pro_relu=s.pro_relu,
                  pro_pool=s.pro_pool, epi_scale=epi_scale, epi_shift=epi_shift, act=s.act, R=Rr, ldc=s.ldc, out_f32=s.out_f32,
                  drop_keep=s.drop_keep, drop_seed=s.drop_seed, sum_groups=s.sum_groups, epi_pool=s.epi_pool)


def start_contents(s, d):
    """sum_groups > 1 adds to C: the case's starting value (small integers, NaN in the padding columns)."""
    if s.sum_groups <= 1:
        return None
    rng = np.random.RandomState(zlib.crc32(s.name.encode()) & 0xFFFF)
    C0 = np.full((d.M, d.ldc), np.nan)
    C0[:, :d.N] = rng.randint(-3, 4, (d.M, d.N))
    return C0


def exactness(s, d):
    """(largest intermediate magnitude, largest stored magnitude, stored values on the grid?) of case s."""
    stored16 = d.dtype == BF16 and not d.out_f32
    if d.mode == HIGHWAY:
        parts = {}
        C = R.conv_gemm(d, round_out=False, parts=parts)[:, :d.Cin]
        big = max(parts['S_h'].max(), parts['S_t'].max()) + 2048.0 + 3.0
        grid = np.all(C * 2 == np.round(C * 2)) and (np.abs(C).max() < 128 if stored16 else True)
        if stored16 and not s.hw_half:
            grid = grid and np.all(C == np.round(C))
        return big, np.abs(C).max(), bool(grid)
    C0 = start_contents(s, d)
    parts = {}
    C = R.conv_gemm(d, C0=C0, round_out=False, parts=parts)
    S = parts['S']
    w = np.isfinite(S)
    sc = np.zeros(d.ldc); sh = np.zeros(d.ldc)
    for g in ([types.SimpleNamespace(c_off=0)] if d.sum_groups else d.groups):
        sc[g.c_off:g.c_off + d.N] = np.abs(R._coef(d.epi_scale, g.c_off, d.N, 1.0))
        sh[g.c_off:g.c_off + d.N] = np.abs(R._coef(d.epi_shift, g.c_off, d.N, 0.0))
    big = (S * sc[None, :] + sh[None, :])[w].max() * (1.0 / min(d.drop_keep, 1.0) if d.drop_keep > 0 else 1.0) + 3.0 + 3.0
    out = C[w]
    grid = np.all(out * 2 == np.round(out * 2))
    if stored16:
        grid = grid and np.all(out == np.round(out))
    return big, np.abs(out).max(), bool(grid)
