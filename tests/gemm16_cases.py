"""Inputs of tests/test_gemm16_kernels_{cpu,gpu}.py: descriptors for vc_gemm16 in the form tests/gemm16_ref.py documents, and
the float32 inputs of the three operand kernels.  numpy only.

EXACT cases hold small integers in BOTH planes (the kernel does not care that lo is small, and a lo plane with integers
of its own makes a wrong plane product show), power-of-two scales, and shifts / old contents on a 1/8 grid, so that every
result is a float32 number and any order of the float32 adds gives the same bits: device == reference, bit for bit.
Every case carries `forced` (option gemm16_split, -1 = default), `ws` ('full' | 'none' | 'small') and `expect`: the
launcher branch it is listed for (test_gemm16_kernels_cpu.py holds the restated launcher rules to it)."""
import functools
import itertools

import numpy as np

import gemm16_ref as R

SENTINEL = 777.0            # outside the stored columns
TAIL = 64                   # elements behind the last output row


def _ints(rng, shape, amp):
    return rng.randint(-amp, amp + 1, size=shape).astype(np.float64)


def planes(rng, M, C, ldx, amp=3):
    """[M, ldx] float16: integer hi and lo planes, NaN in the padding."""
    X = np.full((M, ldx), np.nan, np.float16)
    X[:, :2 * C] = _ints(rng, (M, 2 * C), amp)
    return X


def pair(rng, C, taps0, extra, pad_l, c_off0, c_off1, row0=0, nrows0=0, nrows1=0, s_off0=0, s_off1=0, amp=3, bt1=True):
    return dict(Bt0=_ints(rng, (128, taps0 * 2 * C), amp).astype(np.float16),
                Bt1=_ints(rng, (128, (taps0 + extra) * 2 * C), amp).astype(np.float16) if bt1 else None,
                taps0=taps0, extra=extra, pad_l=pad_l, c_off0=c_off0, c_off1=c_off1, row0=row0, nrows0=nrows0, nrows1=nrows1,
                s_off0=s_off0, s_off1=s_off1)


def ragged_pair(rng, C, single, amp=2):
    n = 2 * R.ragged_pl(C)
    return dict(Bt0=_ints(rng, (128, n), amp).astype(np.float16), Bt1=None if single else _ints(rng, (128, n), amp).astype(np.float16),
                taps0=0, extra=0, pad_l=0, c_off0=0, c_off1=0 if single else 128, row0=0, nrows0=0, nrows1=-1 if single else 0,
                s_off0=0, s_off1=0)


def desc(rng, name, M, T, C, pairs, ldc, ldx=None, rs=True, cs=True, shift=False, accumulate=False, act=0, ragged=False,
         atomic=0, nbuf=None, ncs=None, forced=-1, ws='none', expect=None, X=None, old=None):
    ldx = 2 * C if ldx is None else ldx
    d = dict(name=name, M=M, T=T, C=C, ldx=ldx, X16=planes(rng, M, C, ldx) if X is None else X, pairs=pairs, ldc=ldc,
             ragged=int(ragged), accumulate=int(accumulate), act=act, atomic_splits=atomic, forced=forced, ws=ws, expect=expect or {})
    rows_out = max(max(R.pair_rows(d, p)) for p in pairs)
    d['nbuf'] = rows_out * ldc + TAIL if nbuf is None else nbuf
    ncs = ldc if ncs is None else ncs
    d['row_scale'] = (2.0 ** rng.randint(-2, 3, size=M)).astype(np.float32) if rs else None
    d['col_scale'] = (2.0 ** rng.randint(-2, 2, size=ncs)).astype(np.float32) if cs else None
    d['col_shift'] = (rng.randint(-40, 41, size=ncs) * 0.125).astype(np.float32) if shift else None
    mask = R.stored_mask(d)
    if old is not None:
        d['old'] = old
    elif accumulate or atomic:
        d['old'] = np.where(mask, rng.randint(-64, 65, size=d['nbuf']) * 0.125, 0.0 if atomic else SENTINEL).astype(np.float32)
    else:
        d['old'] = np.where(mask, np.nan, SENTINEL).astype(np.float32)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# exact cases of vc_gemm16

def tap_combos():
    """Every (taps0, extra, pad_l): taps 1..33, extra 0 and 1, pad_l = 0, (k - 1) // 2 and k - 1 of the wider filter k."""
    out = []
    for taps0, extra in itertools.product(range(1, 34), (0, 1)):
        k = taps0 + extra
        if k <= 33:
            out += [(taps0, extra, p) for p in sorted({0, (k - 1) // 2, k - 1})]
    return out


TAP_CHUNK = 15              # pairs per launch of the tap sweep: the plain grid (16 pairs take the per-XCD map)
N_TAP_CASES = -(-len(tap_combos()) // TAP_CHUNK)
ONEHOT = [(f, c, pl) for f in (31, 32, 127, 128, 129, 130) for c in (15, 16, 63, 64) for pl in (0, 1)]
EPI = list(itertools.product((0, 1), (0, 1), (0, 1), ((1, 1), (0, 1), (1, 0))))      # act, shift, accumulate, (row_scale, col_scale)
SPLIT_FORCED = [1, 2, 3, 4, 8, 16 + 2, 16 + 4, 16 + 8]
RAGGED = [(K, H, ws) for K in (2, 3, 8, 32) for H in (256, 128) for ws in ('full', 'none')]
RAGGED_T = {2: (130, 260), 3: (130, 260), 8: (6, 258), 32: (20, 40)}               # K -> (T, M); T = 6 and 20: shorter than the widest bank
RAGGED_KS = {2: 3, 3: 4, 8: 8, 32: 8}


def _gaps(n_pairs, gap=4):
    """Column offsets of n_pairs x 2 filters with `gap` untouched columns between any two, and the pitch."""
    offs = [(i * 2 * (128 + gap), i * 2 * (128 + gap) + 128 + gap) for i in range(n_pairs)]
    return offs, n_pairs * 2 * (128 + gap) + 4


def _build(name):
    rng = np.random.RandomState(abs(hash_name(name)) % (2 ** 31))
    if name == 'rows260':                # a window edge inside a row tile; 4 real rows in the second tile; ldx and ldc with gaps
        offs, ldc = _gaps(2)
        return desc(rng, name, 260, 130, 64, [pair(rng, 64, 3, 1, 1, *offs[0]), pair(rng, 64, 5, 0, 2, *offs[1])], ldc, ldx=2 * 64 + 8,
                    shift=True, expect=dict(form='plain', ntm=2))
    if name == 'm257':                   # one real row in the second tile, one window
        return desc(rng, name, 257, 257, 128, [pair(rng, 128, 5, 0, 2, 0, 128)], 256, expect=dict(form='plain', ntm=2))
    if name == 't3k8':                   # every tap of the wide filter masked somewhere
        return desc(rng, name, 12, 3, 64, [pair(rng, 64, 7, 1, 3, 0, 128)], 256, expect=dict(form='plain', ntm=1))
    if name == 't1':
        return desc(rng, name, 5, 1, 64, [pair(rng, 64, 3, 0, 1, 0, 128)], 256, expect=dict(form='plain', ntm=1))
    if name == 'c192_auto':              # the automatic split; a K range that starts in the middle of a plane
        return desc(rng, name, 260, 130, 192, [pair(rng, 192, 3, 0, 1, 0, 128)], 256, ws='full',
                    expect=dict(form='split', ks=2, split_cs=[0, 5, 9]))
    if name == 'c512_auto':
        return desc(rng, name, 130, 65, 512, [pair(rng, 512, 2, 1, 1, 0, 128, amp=2)], 256, ws='full',
                    expect=dict(form='split', ks=6, split_cs=[0, 4, 8, 12, 16, 20, 24]))
    if name == 'single_null_bt1':        # ONE 128-column filter, d_Bt1 NULL
        return desc(rng, name, 260, 130, 128, [pair(rng, 128, 3, 0, 1, 4, 0, nrows1=-1, bt1=False)], 136, expect=dict(form='plain'))
    if name == 'row0':                   # pairs that walk different row ranges, filters that store different row counts
        offs, ldc = _gaps(2)
        return desc(rng, name, 390, 130, 64, [pair(rng, 64, 3, 1, 1, *offs[0], row0=130, nrows0=260, nrows1=132),
                                              pair(rng, 64, 2, 0, 0, *offs[1], row0=0, nrows0=4, nrows1=0)], ldc, expect=dict(form='plain', ntm=2))
    if name.startswith('taps_'):
        combos = tap_combos()[int(name[5:]) * TAP_CHUNK:][:TAP_CHUNK]
        offs, ldc = _gaps(len(combos), gap=0)
        return desc(rng, name, 72, 36, 64, [pair(rng, 64, t0, ex, pd, *offs[i]) for i, (t0, ex, pd) in enumerate(combos)], ldc,
                    expect=dict(form='plain', ntm=1))
    if name.startswith('onehot_'):       # one 1.0 in one plane at (frame, channel); the output IS a weight (or a sum of two)
        f, c, pl = ONEHOT[int(name[7:])]
        X = np.zeros((260, 256), np.float16)
        X[f, pl * 128 + c] = 1.0
        return desc(rng, name, 260, 130, 128, [pair(rng, 128, 3, 1, 1, 0, 128, amp=1000)], 256, rs=False, cs=False, X=X,
                    expect=dict(form='plain', ntm=2))
    if name.startswith('epi_'):
        act, shift, acc, (rs, cs) = EPI[int(name[4:])]
        return desc(rng, name, 260, 130, 64, [pair(rng, 64, 2, 1, 1, 0, 132)], 264, rs=bool(rs), cs=bool(cs), shift=bool(shift),
                    accumulate=bool(acc), act=act, expect=dict(form='plain'))
    if name.startswith('split_f'):       # 3 row tiles: neither 8 / 2 nor 8 / 4 divides them, so the map has surplus workgroups
        forced = int(name[7:])
        want = forced & 15
        rng = np.random.RandomState(4242)                             # the same data under every forced value
        exp = dict(form='split' if want > 1 else 'plain', ks=want, split_map=int(forced >= 16), ntm=3)
        if forced >= 16:
            exp['idle'] = {2: 8 * 1 - 6, 4: 8 * 2 - 12, 8: 0}[want]
        return desc(rng, name, 520, 130, 384, [pair(rng, 384, 2, 0, 0, 0, 128, amp=2)], 256, shift=True, forced=forced, ws='full', expect=exp)
    if name == 'split_auto':
        rng = np.random.RandomState(4242)
        return desc(rng, name, 520, 130, 384, [pair(rng, 384, 2, 0, 0, 0, 128, amp=2)], 256, shift=True, ws='full',
                    expect=dict(form='split', ks=4, split_map=0))
    if name in ('split_ws_none', 'split_ws_small'):                   # no room for the slabs: one workgroup per row tile
        rng = np.random.RandomState(4242)
        return desc(rng, name, 520, 130, 384, [pair(rng, 384, 2, 0, 0, 0, 128, amp=2)], 256, shift=True, ws=name[9:], expect=dict(form='plain'))
    if name.startswith('rag_'):
        K, H, ws = RAGGED[int(name[4:])]
        T, M = RAGGED_T[K]
        C = 128 * K
        exp = dict(form='split', ks=RAGGED_KS[K]) if ws == 'full' else dict(form='plain')
        X = planes(rng, M, C, 2 * C, amp=2)
        return desc(rng, name, M, T, C, [ragged_pair(rng, C, H == 128)], H, ragged=True, accumulate=True, ws=ws, expect=exp, X=X)
    if name.startswith('p16_ntm') or name in ('p2', 'p15'):
        n, M = (16, 130 * (2 * int(name[7:]) - 1)) if name[1:3] == '16' else (int(name[1:]), 260)
        return desc(rng, name, M, 130, 64, [pair(rng, 64, 1 + i % 4, i & 1, (i % 4) // 2, 256 * i, 256 * i + 128) for i in range(n)],
                    256 * n, expect=dict(form='xcd16' if n == 16 else 'plain', ntm=-(-M // 256)))
    if name.startswith('atomic_z'):      # the weight-gradient form: element offsets, per-pair row ranges, scales from s_off
        zs = int(name[8:])
        M, Cf, ldc, guard = 300, 192, 128, 7
        geo = [(0, 300, 128), (40, 260, 200), (172, 100, 128)]
        pairs, off = [], 61
        for i, (row0, n0, n1) in enumerate(geo):
            o0, o1 = off, off + n0 * ldc + guard
            off = o1 + n1 * ldc + guard
            pairs.append(pair(rng, Cf, 1, 0, 0, o0, o1, row0=row0, nrows0=n0, nrows1=n1, s_off0=128 * (5 - i) + 3, s_off1=64 * i + 1))
        return desc(rng, name, M, M, Cf, pairs, ldc, atomic=zs, nbuf=off + TAIL, ncs=1024,
                    expect=dict(form='atomic', ks=zs, split_cs=[9 * i // zs for i in range(zs + 1)]))
    if name.startswith('nan_'):          # a NaN window between two clean ones ('..._clean': the same data without the NaN)
        kind, clean = name.split('_')[1], name.endswith('_clean')
        rng = np.random.RandomState({'uniform': 11, 'ragged': 12, 'split': 13}[kind])
        if kind == 'ragged':
            C, T, M = 384, 20, 60
            X = planes(rng, M, C, 2 * C, amp=2)
            pairs, kw = [ragged_pair(rng, C, False)], dict(ragged=True, ws='full', expect=dict(form='split', ks=4))
        elif kind == 'split':
            C, T, M = 384, 100, 300
            X = planes(rng, M, C, 2 * C, amp=2)
            pairs, kw = [pair(rng, C, 4, 1, 2, 0, 128, amp=2)], dict(ws='full', expect=dict(form='split', ks=4))
        else:
            C, T, M = 64, 100, 300
            X = planes(rng, M, C, 2 * C)
            pairs, kw = [pair(rng, C, 8, 1, 4, 0, 128), pair(rng, C, 1, 0, 0, 256, 384)], dict(expect=dict(form='plain'))
        if not clean:
            X[T:2 * T] = np.nan
        return desc(rng, name, M, T, C, pairs, 128 * 2 * len(pairs), shift=True, X=X, **kw)
    raise KeyError(name)


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


@functools.lru_cache(maxsize=None)
def get(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 reference output of a case, computed once (read-only: the tests share it)."""
    out = R.gemm16(get(name))
    out.setflags(write=False)
    return out


SHAPES = ['rows260', 'm257', 't3k8', 't1', 'c192_auto', 'c512_auto', 'single_null_bt1', 'row0']
TAPS = ['taps_%d' % i for i in range(N_TAP_CASES)]
ONEHOTS = ['onehot_%d' % i for i in range(len(ONEHOT))]
EPIS = ['epi_%d' % i for i in range(len(EPI))]
SPLITS = ['split_f%d' % f for f in SPLIT_FORCED] + ['split_auto', 'split_ws_none', 'split_ws_small']
RAGGEDS = ['rag_%d' % i for i in range(len(RAGGED))]
PAIRS = ['p16_ntm1', 'p16_ntm2', 'p16_ntm3', 'p2', 'p15']
ATOMICS = ['atomic_z1', 'atomic_z2', 'atomic_z8']
NANS = ['nan_uniform', 'nan_ragged', 'nan_split']
EXACT = SHAPES + TAPS + ONEHOTS + EPIS + SPLITS + RAGGEDS + PAIRS + ATOMICS + NANS + [n + '_clean' for n in NANS]

# ---------------------------------------------------------------------------------------------------------------------
# real-valued cases of vc_gemm16: float32 inputs; the planes come from the device's own vc_split16 / vc_weights16 and the
# reference is taken of THOSE planes.  (name, M, T, C, [(taps0, extra, pad_l)], ragged H or 0, atomic_splits, workspace)
REAL = [('real_c192_split', 260, 130, 192, [(3, 1, 1)], 0, 0, 'full'),
        ('real_33taps', 260, 130, 64, [(33, 0, 16), (1, 1, 0)], 0, 0, 'none'),
        ('real_ragged8', 258, 6, 1024, [], 256, 0, 'full'),
        ('real_atomic', 256, 256, 192, [(1, 0, 0), (1, 0, 0)], 0, 2, 'none')]


def real_inputs(name):
    """-> (X [M, C] float32 with per-window magnitudes over several decades, [W_f [taps, C, 128] float32 per filter])."""
    _, M, T, C, taps, H, zs, ws = next(r for r in REAL if r[0] == name)
    rng = np.random.RandomState(hash_name(name))
    X = (rng.standard_normal((M, C)) * np.exp(2.3 * rng.standard_normal((M // T, 1, 1)).repeat(T, 1).reshape(M, 1))).astype(np.float32)
    if H:
        Ws = [(rng.standard_normal((k, H, 128)) * (0.3 / (k * H) ** 0.5) * (1 + k % 3)).astype(np.float32) for k in range(1, C // 128 + 1)]
    else:
        Ws = [(rng.standard_normal((t0 + ex * f, C, 128)) * 0.05 * (1 + 7 * f)).astype(np.float32) for t0, ex, _ in taps for f in (0, 1)]
    return X, Ws


# ---------------------------------------------------------------------------------------------------------------------
# the operand kernels.  Values sit on a coarse binary grid so that the prologue's fmaf is exact in float64.

def grid_values(rng, shape, bits=12, decades=6):
    """float32 values m * 2^e with |m| < 2^bits: products with power-of-two / small-integer scales stay exact in float64."""
    return (rng.randint(-(1 << bits), 1 << bits, size=shape) * 2.0 ** rng.randint(-decades, decades, size=shape)).astype(np.float32)


# vc_split16: (name, M, T, C, ldx)
SPLIT16_SHAPES = [('c64', 12, 4, 64, 68), ('c192', 10, 5, 192, 196), ('c320', 6, 3, 320, 324), ('c448', 6, 6, 448, 452),
                  ('c1024', 4, 2, 1024, 1028), ('c4096', 3, 1, 4096, 4100), ('t1', 5, 1, 64, 64), ('t_is_m', 7, 7, 128, 128),
                  ('w1100', 2200, 2, 64, 64)]
SPLIT16_TL = {'c64': (4, 1, 4), 'c192': (4, 3, 5), 'c320': (4, 5, 3), 'c448': (4, 7, 6), 'c1024': (8, 1, 2), 'c4096': (8, 4, 1),
              't1': (4, 1, 1), 't_is_m': (5, 1, 7), 'w1100': (4, 1, 1)}


def split16_input(name):
    _, M, T, C, ldx = next(s for s in SPLIT16_SHAPES if s[0] == name)
    rng = np.random.RandomState(hash_name('split16' + name))
    X = np.full((M, ldx), np.nan, np.float32)
    X[:, :C] = grid_values(rng, (M, C)) * (2.0 ** rng.randint(-20, 20, size=(M // T, 1)).repeat(T, 0)).astype(np.float32)
    return X, M, T, C, ldx


def split16_special():
    """[16 windows of T = 3, C = 64]: zero, Inf, NaN, subnormal-only, 2^127 windows with ordinary neighbours, a window with
    values 2^-30 of its maximum (float16-subnormal hi), and a window of tiny values next to one of huge ones."""
    rng = np.random.RandomState(77)
    T, C, nw = 3, 64, 16
    X = grid_values(rng, (nw * T, C)).reshape(nw, T, C)
    X[1] = 0.0
    X[3, 1, 5] = np.inf
    X[5, 2, 63] = np.nan
    X[7] = (rng.randint(-1000, 1000, size=(T, C)) * 2.0 ** -149).astype(np.float32)
    X[9] = rng.randint(-3, 4, size=(T, C)) * np.float32(2.0 ** 125)
    X[9, 0, 0] = 2.0 ** 127
    X[11] = rng.randint(-1023, 1024, size=(T, C)) * np.float32(2.0 ** -40)       # up to 2^-30 of the maximum: hi = m * 2^-26, float16 subnormals
    X[11, 1, 7] = 1.5
    X[13] = rng.randint(-1023, 1024, size=(T, C)) * np.float32(2.0 ** -50)       # below float16's smallest subnormal after scaling
    X[13, 2, 9] = -1.0
    return X.reshape(nw * T, C).astype(np.float32), nw * T, T, C


def prologue_input():
    """M = 12, T = 4, C = 128: scale in {1/2, 1, 2, -1, 3}, shift small integers; window 1's largest magnitude is a
    NEGATIVE value in its last-but-one frame whose successor is larger in value, so the pool removes it (the scale must
    still come from it); window 2 holds its maximum in the last frame (which the pool leaves alone)."""
    rng = np.random.RandomState(78)
    M, T, C = 12, 4, 128
    X = rng.randint(-200, 201, size=(M, C)).astype(np.float32)
    X[T + 2, 17] = -40000.0
    X[2 * T + 3, 3] = 50000.0
    scale = rng.choice([0.5, 1.0, 2.0, -1.0, 3.0], size=C).astype(np.float32)
    scale[17], scale[3] = 1.0, 1.0
    shift = rng.randint(-50, 51, size=C).astype(np.float32)
    return X, M, T, C, scale, shift


# vc_transpose_split16: (name, M, T, C, ldx, shift0, n_shifts)
TRANSPOSE = [('t20_1', 320, 20, 64, 64, -19, 1), ('t20_3', 320, 20, 64, 68, -19, 3), ('t20_32', 320, 20, 192, 192, -19, 32),
             ('t64_64', 320, 64, 64, 64, -63, 64), ('t64_3', 320, 64, 192, 196, -1, 3)]


def transpose_input(name, nan_channel=None):
    _, M, T, C, ldx, s0, ns = next(s for s in TRANSPOSE if s[0] == name)
    rng = np.random.RandomState(hash_name('tr' + name))
    X = np.full((M, ldx), np.nan, np.float32)
    X[:, :C] = grid_values(rng, (M, C)) * (2.0 ** rng.randint(-10, 10, size=(1, C))).astype(np.float32)
    if nan_channel is not None:
        X[2 * T + max(0, -s0 - T + 1), nan_channel] = np.nan      # a frame the first shift reads
    return X, M, T, C, ldx, s0, ns


# vc_weights16: items as tests/gemm16_ref.weights16 takes them; bufs: name -> (dtype, elements)
def weights16_case(name):
    rng = np.random.RandomState(hash_name('w16' + name))
    mk = lambda k, cin, cout, e=0: (grid_values(rng, (k, cin, cout), bits=11, decades=4) * np.float32(2.0 ** e)).astype(np.float32)
    it = lambda src, dst, mode, row_len, tap, plane, base, group, sd=None, so=0, sn=0: dict(
        src=src, dst=dst, k=src.shape[0], cin=src.shape[1], cout=src.shape[2], mode=mode, row_len=row_len, tap_stride=tap,
        plane_stride=plane, base=base, group=group, scale_dst=sd, scale_off=so, scale_n=sn)
    if name == 'mode0':                  # k = 1, 3, 33; cin 32 and 96; cout 40, 128, 256; odd strides, non-zero base
        a, b, c = mk(1, 32, 40), mk(3, 96, 128, 9), mk(33, 32, 256, -7)
        items = [it(a, 'A', 0, 2 * 32 + 10, 2 * 32, 32, 6, 0, 'S', 0, 40),
                 it(b, 'B', 0, 3 * 200 + 8, 200, 100, 4, 1, 'S', 40, 128),
                 it(c, 'C', 0, 33 * 64, 64, 32, 0, 2, None)]
        bufs = dict(A=(np.float16, 40 * 74), B=(np.float16, 128 * 608), C=(np.float16, 256 * 33 * 64), S=(np.float32, 200))
        return items, bufs, 3
    if name == 'mode1':                  # the ragged layout of three banks in one group, items in separate sources
        K, H = 3, 96
        PL = 128 * K * (K + 1) // 2
        srcs = [mk(k, H, 128, 3 * k) for k in range(1, K + 1)]
        items = [it(s, 'A', 1, 2 * PL, 128, PL, 128 * k * (k - 1) // 2, 0, 'S' if k == 1 else None, 0, H if k == 1 else 0)
                 for k, s in enumerate(srcs, 1)]
        d = mk(33, 32, 40)
        items.append(it(d, 'B', 1, 33 * 2 * 48 + 2, 2 * 48, 48, 2, 1, 'S', 100, 32))
        bufs = dict(A=(np.float16, H * 2 * PL), B=(np.float16, 32 * (33 * 96 + 2)), S=(np.float32, 140))
        return items, bufs, 2
    if name == 'groups':                 # one group over two arrays with different strides; an all-zero group; a NaN item
        a, b = mk(3, 32, 128, 5), mk(1, 32, 128, -3)
        z = np.zeros((3, 32, 40), np.float32)
        n = mk(1, 32, 128)
        n[0, 7, 77] = np.nan
        items = [it(a, 'A', 0, 3 * 64, 64, 32, 0, 0, 'S', 0, 128), it(b, 'B', 0, 80, 80, 40, 8, 0, 'S', 128, 64),
                 it(z, 'Z', 0, 3 * 64 + 4, 64, 32, 0, 1, 'S', 192, 40), it(n, 'N', 1, 2 * 128, 256, 128, 0, 2, 'S', 232, 8)]
        bufs = dict(A=(np.float16, 128 * 192), B=(np.float16, 128 * 80), Z=(np.float16, 40 * 196), N=(np.float16, 32 * 256),
                    S=(np.float32, 250))
        return items, bufs, 3
    raise KeyError(name)


WEIGHTS16 = ['mode0', 'mode1', 'groups']
