"""The four launches of csrc/vc_gemm16.hip alone, through the C ABI (_vc.Gemm16Desc, _vc.W16Item; no operand builder of
gemm16.py): vc_gemm16 on hand-made float16 planes, then vc_split16, vc_transpose_split16 and vc_weights16, against the
float64 / bit-model definitions of tests/gemm16_ref.py on the inputs of tests/gemm16_cases.py
(tests/test_gemm16_kernels_cpu.py proves both usable).

Exact cases must EQUAL the reference, bit for bit, over the whole output buffer: it starts as a sentinel outside the
stored columns and as NaN inside them (old contents when the launch accumulates), the ldx padding of the activations
holds NaN, a split-K workspace starts as NaN, and every launch runs twice with identical bits.  Real-valued cases run on
the planes the device's own vc_split16 / vc_weights16 made and are held to the bound gemm16_ref.error_bound derives; a
line starting with MEASURED carries error and bound (profiles/gemm16_kernels/README.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm16_cases as Cs
import gemm16_ref as R
from conftest import poison_gpu_state

pytestmark = pytest.mark.gpu

CAN16, CAN32 = 0x7DA5, 0x7FA5A5A5          # canaries: float16 / float32 NaNs with a payload no arithmetic produces


def _vc():
    import _vc
    return _vc


def _st():
    return _vc().current_stream()


@pytest.fixture(autouse=True)
def _default_split_option():
    poison_gpu_state()
    yield
    _vc().set_option('gemm16_split', -1)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _same_bits(got, want, what):
    """Equal bit for bit; a NaN equals any NaN (payloads are not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & (got.view(u) != want.view(u)))
    if bad.any():
        i = np.flatnonzero(bad.ravel())
        raise AssertionError('%s: %d of %d elements differ, the first at flat index %d: got %r, expected %r'
                             % (what, len(i), bad.size, i[0], got.ravel()[i[0]], want.ravel()[i[0]]))


class Launch:
    """A vc_gemm16 descriptor (tests/gemm16_ref.py's dict form) on the device."""

    def __init__(self, d, workspace=None):
        lib = _vc().lib()
        self.d = d
        self.X = _dev(d['X16'])
        self.rs, self.cs, self.sh = _dev(d['row_scale']), _dev(d['col_scale']), _dev(d['col_shift'])
        self.keep = []
        s = _vc().Gemm16Desc()
        s.d_X16, s.d_row_scale = self.X.data_ptr(), (self.rs.data_ptr() if self.rs is not None else None)
        s.M, s.T, s.C, s.ldx = d['M'], d['T'], d['C'], d['ldx']
        s.n_pairs, s.ragged = len(d['pairs']), d['ragged']
        for i, p in enumerate(d['pairs']):
            b0, b1 = _dev(p['Bt0']), _dev(p['Bt1'])
            self.keep += [b0, b1]
            q = s.pairs[i]
            q.d_Bt0, q.d_Bt1 = b0.data_ptr(), (b1.data_ptr() if b1 is not None else None)
            for k in ('taps0', 'extra', 'pad_l', 'c_off0', 'c_off1', 'row0', 'nrows0', 'nrows1', 's_off0', 's_off1'):
                setattr(q, k, p[k])
        s.d_col_scale = self.cs.data_ptr() if self.cs is not None else None
        s.d_col_shift = self.sh.data_ptr() if self.sh is not None else None
        s.ldc, s.accumulate, s.act, s.atomic_splits = d['ldc'], d['accumulate'], d['act'], d['atomic_splits']
        if workspace is None and d['ws'] != 'none':
            n = lib.vc_gemm16_workspace_bytes(d['M'], d['C'], len(d['pairs'])) if d['ws'] == 'full' else 4096
            assert n == (R.workspace_bytes(d['M'], d['C'], len(d['pairs'])) if d['ws'] == 'full' else 4096)
            workspace = torch.full((n,), 0xFF, dtype=torch.uint8, device='cuda')             # NaN in every slab
        self.ws = workspace
        if workspace is not None:
            s.d_workspace, s.workspace_bytes = workspace.data_ptr(), workspace.numel()
        self.s = s

    def run(self, start=None):
        """One launch into a fresh copy of the case's starting buffer -> the whole buffer on the host."""
        out = _dev(np.asarray(self.d['old'] if start is None else start, np.float32))
        self.s.d_C = out.data_ptr()
        _vc().set_option('gemm16_split', self.d['forced'])
        _vc().check(_vc().lib().vc_gemm16(C.byref(self.s), _st()))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def twice(self):
        a, b = self.run(), self.run()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), '%s: two runs differ' % self.d['name']
        return a


def _exact(name, workspace=None):
    got = Launch(Cs.get(name), workspace).twice()
    _same_bits(got, Cs.reference(name).astype(np.float32), name)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# vc_gemm16, exact

@pytest.mark.parametrize('name', Cs.SHAPES)
def test_row_tiles_windows_and_strides(name):
    _exact(name)


def test_taps_1_to_33_with_every_padding():
    for name in Cs.TAPS:
        _exact(name)


def test_one_hot_placement_at_fragment_tile_and_window_seams():
    for name in Cs.ONEHOTS:
        _exact(name)


def test_epilogue_combinations():
    for name in Cs.EPIS:
        got = _exact(name)
        if Cs.get(name)['act'] == R.ACT_RELU and not Cs.get(name)['accumulate']:
            m = R.stored_mask(Cs.get(name))
            assert (got[m] == 0).any() and got[m].min() >= 0                     # negative results met the relu


def test_split_k_forced_and_automatic_equal_the_unsplit_launch():
    base = _exact('split_f1')
    for name in Cs.SPLITS[1:]:
        _same_bits(_exact(name), base, name + ' against the unsplit launch')


def test_split_k_workspace_reused_across_shapes_and_refused_when_misaligned():
    n = _vc().lib().vc_gemm16_workspace_bytes(520, 384, 1)
    ws = torch.full((n + 256,), 0xFF, dtype=torch.uint8, device='cuda')
    for name in ('split_f8', 'c192_auto', 'rag_0', 'split_f20', 'c512_auto', 'split_f3'):    # each finds the other's slabs and tickets
        _exact(name, ws[:n])
    L = Launch(Cs.get('split_f2'), ws[16:16 + n])
    out = _dev(Cs.get('split_f2')['old'])
    L.s.d_C = out.data_ptr()
    _vc().set_option('gemm16_split', 2)
    rc = _vc().lib().vc_gemm16(C.byref(L.s), _st())
    torch.cuda.synchronize()
    assert rc != 0 and b'256-byte aligned' in _vc().lib().vc_last_error()
    _same_bits(out.cpu().numpy(), Cs.get('split_f2')['old'], 'output of a refused launch')


@pytest.mark.parametrize('name', Cs.RAGGEDS, ids=['K%d_H%d_ws_%s' % r for r in Cs.RAGGED])
def test_ragged_walk(name):
    _exact(name)


@pytest.mark.parametrize('name', Cs.PAIRS)
def test_pair_grids(name):
    _exact(name)


@pytest.mark.parametrize('name', Cs.ATOMICS)
def test_atomic_splits_scatter(name):
    got = _exact(name)
    assert not got[~R.stored_mask(Cs.get(name))].any()                           # guards before and after every block stay zero


@pytest.mark.parametrize('name', Cs.NANS)
def test_nan_window_does_not_leak(name):
    d = Cs.get(name)
    dirty, clean = _exact(name), _exact(name + '_clean')
    rows = np.arange(d['M'])
    keep = np.repeat((rows < d['T']) | (rows >= 2 * d['T']), d['ldc'])
    assert np.isnan(dirty[:d['M'] * d['ldc']][~keep]).all()
    _same_bits(dirty[:d['M'] * d['ldc']][keep], clean[:d['M'] * d['ldc']][keep], name + ': clean windows')


def _reject(d, text, **edit):
    L = Launch(d)
    out = _dev(d['old'])
    L.s.d_C = out.data_ptr()
    pair_edit = {k[5:]: v for k, v in edit.items() if k.startswith('pair_')}
    for k, v in edit.items():
        if not k.startswith('pair_'):
            setattr(L.s, k, v(L) if callable(v) else v)
    for k, v in pair_edit.items():
        setattr(L.s.pairs[0], k, v)
    _vc().set_option('gemm16_split', d['forced'])
    rc = _vc().lib().vc_gemm16(C.byref(L.s), _st())
    torch.cuda.synchronize()
    msg = _vc().lib().vc_last_error().decode()
    assert rc != 0 and text in msg, (text, rc, msg)
    if 'd_C' not in edit:
        _same_bits(out.cpu().numpy(), d['old'], 'output of the launch refused for "%s"' % text)


def test_every_requirement_of_the_launcher_refuses():
    d, at, sp = Cs.get('epi_0'), Cs.get('atomic_z2'), Cs.get('c192_auto')
    _reject(d, 'NULL argument', d_X16=None)
    _reject(d, 'NULL argument', d_C=None)
    _reject(d, 'bad shape', T=7)
    _reject(d, 'bad pair count / ldc', n_pairs=0)
    _reject(d, 'act must be none or relu', act=2)
    _reject(at, 'atomic_splits 0..8', atomic_splits=9)
    _reject(d, 'unaligned', d_X16=lambda L: L.X.data_ptr() + 2)
    _reject(d, 'ragged walk needs one pair', ragged=1)
    _reject(d, 'NULL / unaligned weights', pair_d_Bt0=None)
    _reject(d, 'NULL / unaligned weights', pair_d_Bt1=None)                      # NULL only where nrows1 = -1 says it is not read
    _reject(d, 'bad output columns', pair_c_off0=2)
    _reject(d, 'bad row range', pair_nrows0=d['M'] + 1)
    _reject(d, 'bad taps', pair_pad_l=3)
    _reject(at, 'more K ranges than K slabs', C=64, ldx=384, atomic_splits=4)
    _reject(sp, '256-byte aligned', d_workspace=lambda L: L.ws.data_ptr() + 16, workspace_bytes=lambda L: L.ws.numel() - 16)


# ---------------------------------------------------------------------------------------------------------------------
# the operand kernels, bit for bit

def _split16(X, M, Cn, ldx, T, scale=None, shift=None, relu=0, pool=0):
    """-> (out16 [M, 2 Cn] float16, row_scale [M] float32); canaries behind both must survive (the M / T scratch words excepted)."""
    x = _dev(X)
    out = torch.full((M * 2 * Cn + 64,), CAN16, dtype=torch.int16, device='cuda')
    rs = torch.full((M + M // T + 64,), CAN32, dtype=torch.int32, device='cuda')
    sc, sh = _dev(scale), _dev(shift)
    _vc().check(_vc().lib().vc_split16(_p(x), M, Cn, ldx, T, _p(sc), _p(sh), relu, pool, _p(out), _p(rs), _st()))
    torch.cuda.synchronize()
    assert bool((out[M * 2 * Cn:] == CAN16).all()) and bool((rs[M + M // T:] == CAN32).all()), 'wrote behind its outputs'
    return out[:M * 2 * Cn].view(torch.float16).view(M, 2 * Cn).cpu().numpy(), rs[:M].view(torch.float32).cpu().numpy()


def _check_split16(X, M, T, Cn, ldx, what, **pro):
    got16, got_rs = _split16(X, M, Cn, ldx, T, **pro)
    want16, want_rs = R.split16(X, Cn, T, **pro)
    _same_bits(got_rs, want_rs, what + ': row_scale')
    _same_bits(got16, want16, what + ': planes')
    return got16, got_rs


@pytest.mark.parametrize('name', [s[0] for s in Cs.SPLIT16_SHAPES])
def test_split16_shapes(name):
    X, M, T, Cn, ldx = Cs.split16_input(name)
    _check_split16(X, M, T, Cn, ldx, 'vc_split16 ' + name)


def test_split16_special_windows_leave_their_neighbours_alone():
    X, M, T, Cn = Cs.split16_special()
    got16, rs = _check_split16(X, M, T, Cn, Cn, 'vc_split16 special windows')
    assert rs[1 * T] == 1 and rs[3 * T] == 1 and rs[5 * T] == 1 and rs[7 * T] == 2.0 ** -114 and rs[9 * T] == 2.0 ** 113
    sub = np.abs(got16[11 * T:12 * T, :Cn].astype(np.float64))
    assert ((sub > 0) & (sub < 2.0 ** -14)).any(), 'no float16-subnormal hi came out: flushed?'


def test_split16_prologue_in_every_combination():
    X, M, T, Cn, scale, shift = Cs.prologue_input()
    for sc in (None, scale):
        for sh in (None, shift):
            for relu in (0, 1):
                for pool in (0, 1):
                    _check_split16(X, M, T, Cn, Cn, 'vc_split16 prologue scale=%d shift=%d relu=%d pool=%d' % (sc is not None, sh is not None, relu, pool),
                                   scale=sc, shift=sh, relu=relu, pool=pool)
    # the window whose largest magnitude the pool removes keeps the scale of that magnitude
    got16, rs = _split16(X, M, Cn, Cn, T, pool=1)
    assert rs[T] == 2.0 ** (15 - 14) and np.abs(got16[T:2 * T, :Cn].astype(np.float64)).max() < 2.0 ** 13


def _transpose(X, M, Cn, ldx, T, s0, ns, scale=None, shift=None, relu=0, pool=0):
    x = _dev(X)
    out = torch.full((ns * Cn * 2 * M + 64,), CAN16, dtype=torch.int16, device='cuda')
    rs = torch.full(((ns + 1) * Cn + 64,), CAN32, dtype=torch.int32, device='cuda')
    sc, sh = _dev(scale), _dev(shift)
    _vc().check(_vc().lib().vc_transpose_split16(_p(x), M, Cn, ldx, T, _p(sc), _p(sh), relu, pool, s0, ns, _p(out), _p(rs), _st()))
    torch.cuda.synchronize()
    assert bool((out[ns * Cn * 2 * M:] == CAN16).all()) and bool((rs[(ns + 1) * Cn:] == CAN32).all()), 'wrote behind its outputs'
    return out[:ns * Cn * 2 * M].view(torch.float16).view(ns * Cn, 2 * M).cpu().numpy(), rs[:ns * Cn].view(torch.float32).cpu().numpy()


@pytest.mark.parametrize('name', [s[0] for s in Cs.TRANSPOSE])
def test_transpose_split16(name):
    for nan_channel, pro in ((None, {}), (None, 'pool'), (33, {})):
        X, M, T, Cn, ldx, s0, ns = Cs.transpose_input(name, nan_channel)
        if pro == 'pool':
            rng = np.random.RandomState(5)
            pro = dict(scale=rng.choice([0.5, 1.0, -2.0], size=Cn).astype(np.float32), shift=rng.randint(-8, 9, size=Cn).astype(np.float32),
                       relu=1, pool=1)
        got16, got_rs = _transpose(X, M, Cn, ldx, T, s0, ns, **pro)
        want16, want_rs = R.transpose_split16(X, Cn, T, s0, ns, **pro)
        what = 'vc_transpose_split16 %s%s%s' % (name, ' with the prologue' if pro else '', ' with a NaN channel' if nan_channel else '')
        _same_bits(got_rs, want_rs, what + ': row_scale of every shift')
        _same_bits(got16, want16, what + ': rows')
        if nan_channel is not None:
            assert np.isnan(got16[nan_channel]).any() and not np.isnan(np.delete(got16[:Cn], nan_channel, 0)).any()


@pytest.mark.parametrize('name', Cs.WEIGHTS16)
def test_weights16(name):
    items, bufs, n_groups = Cs.weights16_case(name)
    host = {k: np.full(n, np.nan, dt) for k, (dt, n) in bufs.items()}
    dev = {k: (torch.full((n + 64,), CAN16, dtype=torch.int16, device='cuda') if dt == np.float16 else
               torch.full((n + 64,), CAN32, dtype=torch.int32, device='cuda')) for k, (dt, n) in bufs.items()}
    srcs = [_dev(it['src']) for it in items]
    tab = (_vc().W16Item * len(items))()
    for t, it, s in zip(tab, items, srcs):
        t.src, t.dst = s.data_ptr(), dev[it['dst']].data_ptr()
        t.scale_dst = dev[it['scale_dst']].data_ptr() + 4 * it['scale_off'] if it['scale_dst'] is not None else None
        for k in ('k', 'cin', 'cout', 'mode', 'row_len', 'tap_stride', 'plane_stride', 'base', 'group', 'scale_n'):
            setattr(t, k, it[k])
    d_tab = torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda()
    gmax = torch.full((n_groups,), -1, dtype=torch.int32, device='cuda')
    _vc().check(_vc().lib().vc_weights16(_p(d_tab), len(items), _p(gmax), n_groups, _st()))
    torch.cuda.synchronize()
    want = R.weights16(items, host, n_groups)
    other = R.weights16(items, {k: np.ones(n, dt) for k, (dt, n) in bufs.items()}, n_groups)
    for k, (dt, n) in bufs.items():
        raw = dev[k].cpu().numpy()
        can = CAN16 if dt == np.float16 else CAN32
        u = np.uint16 if dt == np.float16 else np.uint32
        assert (raw[n:] == can).all(), 'vc_weights16 %s: wrote behind buffer %s' % (name, k)
        hole = want[k].view(u) != other[k].view(u)            # what the reference leaves as it found it
        assert (raw[:n][hole] == can).all(), 'vc_weights16 %s: wrote between the extents of buffer %s' % (name, k)
        got = raw[:n].view(dt).copy()
        _same_bits(np.where(hole, dt(0), got), np.where(hole, dt(0), want[k]), 'vc_weights16 %s buffer %s' % (name, k))


# ---------------------------------------------------------------------------------------------------------------------
# vc_gemm16 on real values: the device's own planes, the derived bound

@pytest.mark.parametrize('case', Cs.REAL, ids=[r[0] for r in Cs.REAL])
def test_real_values_stay_inside_the_derived_bound(case):
    name, M, T, Cn, taps, H, zs, ws = case
    X, Ws = Cs.real_inputs(name)
    x16, rs = _split16(X, M, Cn, Cn, T)
    n_pairs = 1 if H else len(taps)
    ldc = H if H else 256 * n_pairs
    cs = torch.full((ldc,), CAN32, dtype=torch.int32, device='cuda')
    srcs = [_dev(W) for W in Ws]
    tab = (_vc().W16Item * len(Ws))()
    if H:
        PL = R.ragged_pl(Cn)
        bt = [torch.full((H, 2 * PL), CAN16, dtype=torch.int16, device='cuda')]
        for k, (t, s) in enumerate(zip(tab, srcs), 1):
            t.src, t.dst, t.scale_dst = s.data_ptr(), bt[0].data_ptr(), (cs.data_ptr() if k == 1 else None)
            t.k, t.cin, t.cout, t.mode, t.row_len, t.tap_stride, t.plane_stride, t.base = k, H, 128, 1, 2 * PL, 128, PL, 128 * k * (k - 1) // 2
            t.group, t.scale_n = 0, (H if k == 1 else 0)
        n_groups = 1
    else:
        bt = [torch.full((128, W.shape[0] * 2 * Cn), CAN16, dtype=torch.int16, device='cuda') for W in Ws]
        for i, (t, s, W) in enumerate(zip(tab, srcs, Ws)):
            t.src, t.dst, t.scale_dst = s.data_ptr(), bt[i].data_ptr(), cs.data_ptr() + 4 * 128 * i
            t.k, t.cin, t.cout, t.mode, t.row_len, t.tap_stride, t.plane_stride, t.base = W.shape[0], Cn, 128, 0, W.shape[0] * 2 * Cn, 2 * Cn, Cn, 0
            t.group, t.scale_n = i, 128
        n_groups = len(Ws)
    d_tab = torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda()
    gmax = torch.empty(n_groups, dtype=torch.int32, device='cuda')
    _vc().check(_vc().lib().vc_weights16(_p(d_tab), len(Ws), _p(gmax), n_groups, _st()))
    torch.cuda.synchronize()
    bth = [b.view(torch.float16).cpu().numpy() for b in bt]
    assert not any(np.isnan(b).any() for b in bth)
    if H:
        pairs = [dict(Bt0=bth[0][:128], Bt1=bth[0][128:], taps0=0, extra=0, pad_l=0, c_off0=0, c_off1=128, row0=0, nrows0=0, nrows1=0, s_off0=0, s_off1=128)]
    else:
        pairs = [dict(Bt0=bth[2 * i], Bt1=bth[2 * i + 1], taps0=t0, extra=ex, pad_l=pd, c_off0=256 * i, c_off1=256 * i + 128, row0=0, nrows0=0,
                      nrows1=0, s_off0=256 * i, s_off1=256 * i + 128) for i, (t0, ex, pd) in enumerate(taps)]
    d = dict(name=name, M=M, T=T, C=Cn, ldx=2 * Cn, X16=x16, row_scale=rs, col_scale=cs.view(torch.float32).cpu().numpy(), col_shift=None,
             pairs=pairs, ldc=ldc, ragged=int(bool(H)), accumulate=0, act=0, atomic_splits=zs, forced=-1, ws=ws, expect={}, nbuf=M * ldc + Cs.TAIL)
    mask = R.stored_mask(d)
    d['old'] = np.where(mask, 0.0 if zs else np.nan, Cs.SENTINEL).astype(np.float32)
    L = Launch(d)
    got = L.run() if zs else L.twice()                  # (the atomic form's order of adds is not fixed)
    ref, bound = R.gemm16(d), R.error_bound(d)
    assert np.array_equal(got[~mask], d['old'][~mask])
    err = np.abs(got.astype(np.float64) - ref)[mask]
    ratio = err / bound[mask]
    i = int(np.argmax(ratio))
    print('\nMEASURED %s: worst error / bound %.4f (error %.3e, bound %.3e, result %.3e); largest error %.3e; n = %d products'
          % (name, ratio[i], err[i], bound[mask][i], ref[mask][i], err.max(), R.products_per_output(d, pairs[0], False)))
    assert (err <= bound[mask]).all(), (name, float(ratio.max()))
