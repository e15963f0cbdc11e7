"""The postfilters on the MI355X: the four launches of csrc/vc_postfilter.hip alone through the C ABI against
tests/postfilter_ref.py, their exact properties, graph replay, refusals, and conversion.convert_postfilter_batch.

Every kernel call as tests/test_diff_gpu.py makes them: every buffer inside sentinel bands that are checked after the call,
outputs filled with NaN before it, input rows at or beyond an utterance's frame count NaN (a kernel that read one would
show it), max_frames odd and larger than every count.

Bounds.  Mean, variance and the modulation-spectrum sums have Higham-style bounds for the documented summation order
(_stats_bound, _ms_bounds).  Both filters are held to 4 times the float32 twin's own worst distance from float64 on the
same inputs, and never to less than 4 roundings of the output value itself (4 * 2^-24 |y|): on an array of a handful of
elements the twin can land on the float64 value by luck, and no float32 computation can promise that."""
import contextlib
import io

import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import postfilter_ref as pr
from test_convert_batch_gpu import _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)

pytestmark = pytest.mark.gpu

BAND = 1024
SENT = np.float32(-98765.4375)
NAN = float('nan')
U = 2.0 ** -24
FS = (1, 2, 31, 32, 33, 63, 64, 65, 97, 129)
CS = (1, 63, 64, 65, 80, 201)
HI = 20.0 * np.log(10.0) / 20.0
N_ITER = 4


@pytest.fixture(autouse=True)
def _poisoned():
    poison_gpu_state()


class Guarded:
    """n float32 inside a larger device buffer whose bands hold the sentinel; .t is the inner view."""

    def __init__(self, n, fill=float(SENT), host=None):
        self.full = torch.full((n + 2 * BAND,), float(SENT), dtype=torch.float32, device='cuda')
        self.t = self.full[BAND:BAND + n]
        if host is not None:
            self.t.copy_(torch.from_numpy(np.array(host, dtype=np.float32).reshape(-1)))
        elif fill != float(SENT):
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.full[:BAND] == float(SENT)).all()) and bool((self.full[-BAND:] == float(SENT)).all()), \
            'sentinel band overwritten around ' + what

    def numpy(self):
        return self.t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _worst(what, got, want, bound):
    """The worst error / bound over all elements (an element whose bound is 0 must be exact); asserts it is at most 1."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape and got.size > 0
    assert np.isfinite(got).all(), what + ': the device value is not finite'
    err = np.abs(got - want)
    zero = bound <= 0.0
    assert not err[zero].any(), what + ': an element with bound 0 is not exact'
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[i] <= 1.0, '%s: error %.3e > bound %.3e at %s' % (what, err[i], bound[i], i)
    return float(ratio[i])


OUT_SIZE = {'stats': lambda B, F, C: B * C * 2, 'gv': lambda B, F, C: B * F * C, 'mss': lambda B, F, C: B * C * pr.M * 3,
            'msf': lambda B, F, C: B * F * C}
OUT_SHAPE = {'stats': lambda B, F, C: (B, C, 2), 'gv': lambda B, F, C: (B, F, C), 'mss': lambda B, F, C: (B, C, pr.M, 3),
             'msf': lambda B, F, C: (B, F, C)}


def _call(kind, x, nf, stats=None, table=None, s0=0.0, s1=0.0, null=None, shape=None, alias=False):
    """One call of a launch on guarded buffers: (rc, the output as the device left it, NaN where unwritten).
    kind: 'stats' (vc_traj_stats_f32), 'gv' (table = gv_t, s0 = alpha, s1 = g_max), 'mss' (vc_ms_stats_f32),
    'msf' (table = coef, s0 = lo, s1 = hi).  null: the name of a pointer to pass as NULL; shape: (batch, max_frames,
    channels) to pass instead of x's; alias: the output pointer is the input's."""
    import _vc
    lib = _vc.lib()
    B, F, C = x.shape
    bufs = {'x': Guarded(x.size, host=x), 'out': Guarded(OUT_SIZE[kind](B, F, C), fill=NAN)}
    if stats is not None:
        bufs['stats'] = Guarded(stats.size, host=stats)
    if table is not None:
        bufs['table'] = Guarded(table.size, host=table)
    d_nf = None if nf is None else torch.tensor([int(v) for v in nf], dtype=torch.int32, device='cuda')
    p = {k: _vc.ptr(v.t) for k, v in bufs.items()}
    if alias:
        p['out'] = p['x']
    if null:
        p[null] = None
    sh = [int(v) for v in (shape or (B, F, C))]
    st = _vc.current_stream()
    if kind == 'stats':
        rc = lib.vc_traj_stats_f32(p['x'], _vc.ptr(d_nf), *sh, p['out'], st)
    elif kind == 'gv':
        rc = lib.vc_gv_filter_f32(p['x'], _vc.ptr(d_nf), p['stats'], p['table'], *sh, float(s0), float(s1), p['out'], st)
    elif kind == 'mss':
        rc = lib.vc_ms_stats_f32(p['x'], _vc.ptr(d_nf), p['stats'], *sh, p['out'], st)
    else:
        rc = lib.vc_ms_filter_f32(p['x'], _vc.ptr(d_nf), p['stats'], p['table'], *sh, float(s0), float(s1), p['out'], st)
    torch.cuda.synchronize()
    for k, g in bufs.items():
        g.check(kind + ' ' + k)
    for k, host in (('x', x), ('stats', stats), ('table', table)):
        if host is not None:
            assert _same_bits(bufs[k].numpy(), np.asarray(host, np.float32).reshape(-1)), 'input %s was written' % k
    return rc, bufs['out'].numpy().reshape(OUT_SHAPE[kind](B, F, C))


def _traj(rng, n, C):
    """[n, C] float32 in (0, 0.9): a two-tap moving average of noise around 0.45, the deviation growing with the channel."""
    z = rng.standard_normal((n + 1, C))
    x = 0.45 + np.linspace(0.03, 0.09, C) * (0.7 * z[1:] + 0.7 * z[:-1])
    return np.clip(x, 0.01, 0.89).astype(np.float32)


def _case(F, C, seed):
    """A ragged batch of 5 with one empty utterance; the longest has F frames; rows at or beyond a count are NaN."""
    rng = np.random.default_rng(1000 * seed + 7 * F + C)
    nf = [F, 0, (F + 1) // 2, max(F - 1, 1), F]
    maxF = F + 3 if F % 2 == 0 else F + 2
    x = np.full((5, maxF, C), NAN, np.float32)
    for b, n in enumerate(nf):
        x[b, :n] = _traj(rng, n, C)
    return x, nf


def _alone(x, nf, b):
    """Utterance b of a case as a batch of one under another max_frames."""
    n = nf[b]
    return np.ascontiguousarray(x[b:b + 1, :n + 2]), [n]


def _rows_beyond_are_zero(y, nf):
    for b, n in enumerate(nf):
        n = min(max(int(n), 0), y.shape[1])
        assert not np.isnan(y[b]).any() and not y[b, n:].any(), 'rows at or beyond n are not 0 (utterance %d)' % b


# ------------------------------------------------------------------------------------------ bounds
def _stats_bound(x, nf, want):
    """Mean: n differences from the first frame (one rounding each), summed in 8 interleaved chains of ceil(n / 8) terms and
    one of 8 -- at most k = ceil(n / 8) + 7 additions over any term -- one division, one addition to the first frame:
    (k + 3) u sum|d| / n + u |mean|.  Variance: every term carries the difference's, the square's and the chain's roundings,
    then one division, (k + 5) u V; V is taken about the ROUNDED mean, which adds (mean error)^2 exactly."""
    B, maxF, C = x.shape
    bm, bv = np.zeros((B, C)), np.zeros((B, C))
    for b, n in enumerate(pr.clamp_n(nf, B, maxF)):
        if n == 0:
            continue
        xb = x[b, :n].astype(np.float64)
        k = (n + pr.ST_WAVES - 1) // pr.ST_WAVES + pr.ST_WAVES - 1
        bm[b] = (k + 3) * U * np.abs(xb - xb[0]).sum(0) / n + U * np.abs(want[b, :, 0])
        bv[b] = (k + 5) * U * (want[b, :, 1] + bm[b] ** 2) + bm[b] ** 2
    return bm, bv


def _ms_bounds(x, nf, stats):
    """Intervals [lo, hi] for vc_ms_stats_f32's [B, C, 33, 3] and the mask of entries all of whose segments are certain.
    A bin of a segment: the device's transform is a sum over the 64 windowed values v_t in which no term passes more than
    16 roundings (window and difference 2; two radix-4 stages 4; three twiddle products with rounded constants 3 each; the
    joins and the untangling 3), so Re and Im each lie within eX = 32 u sum|v_t| of float64's (a factor 2 for the
    complex products' two terms).  From that: p = |X|^2 within rel = (2 sqrt2 eX |X| + 2 eX^2) / |X|^2 + 3 u relatively, and
    s = logf(p) within es = -log(1 - rel) + 2 u |s|.  A segment is CERTAIN to be counted where |X| > 16 eX and p (1 - rel) is
    above the floor, certain not to be where (|X| + 2 eX)^2 is not above it, and UNSURE otherwise -- bins that hold nothing
    but the transform's own rounding, e.g. every bin from 2 up of the last segment of an utterance of 32 k + 1 frames, which
    is the held last frame under the window.  An unsure segment may add nothing, or one count and an s anywhere between
    ln(floor) and ln((|X| + 2 eX)^2).  The sums run in 4 interleaved chains and one of 4: (k + 1) u sum|term| with
    k = ceil(segments / 4) + 3."""
    B, maxF, C = x.shape
    lo, hi = np.zeros((B, C, pr.M, 3)), np.zeros((B, C, pr.M, 3))
    certain = np.ones((B, C, pr.M), bool)
    sl = np.log(pr.FLOOR)
    for b, n in enumerate(pr.clamp_n(nf, B, maxF)):
        if n == 0:
            continue
        v, re, im = pr.spectra(x[b, :n], stats[b, :, 0])
        eX = 32.0 * U * np.abs(v).sum(1)[:, None, :]
        p = re * re + im * im
        mag = np.sqrt(p)
        with np.errstate(all='ignore'):
            rel = np.where(p > 0, (2.0 * np.sqrt(2.0) * eX * mag + 2.0 * eX * eX) / np.where(p > 0, p, 1.0), np.inf) + 3 * U
            sure = (mag > 16.0 * eX) & (p * (1.0 - rel) > pr.FLOOR) & (rel < 0.5)
            never = (mag + 2.0 * eX) ** 2 * (1.0 + 4 * U) <= pr.FLOOR
            unsure = ~sure & ~never
            s = np.where(sure, np.log(np.where(sure, p, 1.0)), 0.0)
            es = np.where(sure, -np.log1p(-np.where(sure, rel, 0.0)) + 2 * U * np.abs(s), 0.0)
            su = np.where(unsure, np.log(np.maximum((mag + 2.0 * eX) ** 2 * (1.0 + 4 * U), pr.FLOOR)), sl)
        gam = ((len(v) + pr.MS_WAVES - 1) // pr.MS_WAVES + pr.MS_WAVES) * U
        t1 = (np.abs(s) + es).sum(0) + (unsure * abs(sl)).sum(0)
        t2_hi = (((np.abs(s) + es) ** 2).sum(0) + (unsure * np.maximum(sl * sl, su * su)).sum(0)) * (1 + U)
        t2_lo = (np.maximum(np.abs(s) - es, 0.0) ** 2).sum(0) * (1 - U)
        cnt = sure.sum(0)
        lo[b, :, :, 0], hi[b, :, :, 0] = cnt.T, (cnt + unsure.sum(0)).T
        lo[b, :, :, 1] = ((s - es).sum(0) + (unsure * min(sl, 0.0)).sum(0) - gam * t1).T
        hi[b, :, :, 1] = ((s + es).sum(0) + (unsure * np.maximum(su, 0.0)).sum(0) + gam * t1).T
        lo[b, :, :, 2], hi[b, :, :, 2] = (t2_lo - gam * t2_hi).T, (t2_hi * (1 + gam)).T
        certain[b] = ~unsure.any(0).T
    return lo, hi, certain


def _twin_bound(want, twin):
    return np.maximum(4.0 * np.abs(twin.astype(np.float64) - want).max(), 4.0 * U * np.abs(want))


# ------------------------------------------------------------------------------------------ the shapes
@pytest.mark.parametrize('C', CS)
def test_traj_stats_shapes(C):
    """F in 1 .. 129 x this C, as a ragged batch of 5 with an empty utterance: mean and variance within their bounds, the
    empty utterance's exactly 0, and every utterance alone -- batch of 1, another max_frames -- bit-identical."""
    worst = [0.0, 0.0]
    for F in FS:
        x, nf = _case(F, C, 1)
        rc, got = _call('stats', x, nf)
        assert rc == 0
        want = pr.traj_stats(x, nf)
        bm, bv = _stats_bound(x, nf, want)
        worst[0] = max(worst[0], _worst('mean F=%d' % F, got[:, :, 0], want[:, :, 0], bm))
        worst[1] = max(worst[1], _worst('variance F=%d' % F, got[:, :, 1], want[:, :, 1], bv))
        assert not got[1].any() and (got[:, :, 1] >= 0).all()
        if F == 1:
            assert _same_bits(got[0, :, 0], x[0, 0]) and not got[:, :, 1].any()
        for b in range(5):
            xa, na = _alone(x, nf, b)
            rc, one = _call('stats', xa, na)
            assert rc == 0 and _same_bits(one[0], got[b]), 'utterance %d alone differs (F=%d)' % (b, F)
    rc, got = _call('stats', x[:, :, :], None)                        # NULL counts: every row counts, NaN rows included
    assert rc == 0 and np.isnan(got[1]).all()
    print('MEASURED traj_stats C=%d: worst fraction of the bound: mean %.3f, variance %.3f' % (C, worst[0], worst[1]))


@pytest.mark.parametrize('C', CS)
def test_gv_filter_shapes(C):
    worst = 0.0
    for F in FS:
        x, nf = _case(F, C, 2)
        stats = pr.traj_stats(x, nf, np.float32)
        rng = np.random.default_rng(F * 31 + C)
        gv_t = (np.maximum(stats[0, :, 1], 1e-4) * rng.uniform(0.3, 3.0, C)).astype(np.float32)
        gv_t[rng.integers(0, C)] = 0.0
        rc, got = _call('gv', x, nf, stats, gv_t, 0.7, 4.0)
        assert rc == 0
        _rows_beyond_are_zero(got, nf)
        want, twin = pr.gv_filter(x, nf, stats, gv_t, 0.7, 4.0), pr.gv_filter(x, nf, stats, gv_t, 0.7, 4.0, np.float32)
        worst = max(worst, _worst('gv F=%d' % F, got, want, _twin_bound(want, twin)))
        for b in range(5):
            xa, na = _alone(x, nf, b)
            rc, one = _call('gv', xa, na, stats[b:b + 1], gv_t, 0.7, 4.0)
            assert rc == 0 and _same_bits(one[0, :nf[b]], got[b, :nf[b]]), 'utterance %d alone differs (F=%d)' % (b, F)
    print('MEASURED gv_filter C=%d: worst fraction of 4 x the twin\'s error: %.3f' % (C, worst))


@pytest.mark.parametrize('C', CS)
def test_ms_stats_shapes(C):
    worst, n_certain, n_all = 0.0, 0, 0
    for F in FS:
        x, nf = _case(F, C, 3)
        stats = pr.traj_stats(x, nf, np.float32)
        rc, got = _call('mss', x, nf, stats)
        assert rc == 0 and np.isfinite(got).all() and not got[1].any()
        lo, hi, certain = _ms_bounds(x, nf, stats)
        assert np.array_equal(got[..., 0], np.rint(got[..., 0]))
        bad = (got < lo) | (got > hi)
        assert not bad.any(), 'F=%d: %d values outside their interval, first at %s: %r not in [%r, %r]' % (
            F, int(bad.sum()), tuple(np.argwhere(bad)[0]), got[bad][0], lo[bad][0], hi[bad][0])
        half = 0.5 * (hi - lo)[certain][:, 1:]
        frac = np.abs(got[certain][:, 1:] - 0.5 * (hi + lo)[certain][:, 1:]) / np.where(half > 0, half, 1.0)
        worst = max(worst, float(frac.max()) if frac.size else 0.0)
        assert np.array_equal(got[certain][:, 0], lo[certain][:, 0])
        n_certain, n_all = n_certain + int(certain.sum()), n_all + certain.size
        if F == 1:
            assert not got.any()                                     # one frame: every deviation is an exact 0
        if F == 64:
            assert certain[0].mean() > 0.9                           # no held tail: (nearly) every bin of every segment is certain
            assert (got[0, :, :, 0] == 3).mean() > 0.9
        for b in range(5):
            xa, na = _alone(x, nf, b)
            rc, one = _call('mss', xa, na, stats[b:b + 1])
            assert rc == 0 and _same_bits(one[0], got[b]), 'utterance %d alone differs (F=%d)' % (b, F)
    assert n_certain > 0.4 * n_all
    print('MEASURED ms_stats C=%d: worst fraction of the interval\'s half width over the %d of %d entries without an unsure '
          'segment: %.3f' % (C, n_certain, n_all, worst))


@pytest.mark.parametrize('C', CS)
def test_ms_filter_shapes(C):
    worst = 0.0
    for F in FS:
        x, nf = _case(F, C, 4)
        stats = pr.traj_stats(x, nf, np.float32)
        rng = np.random.default_rng(F * 37 + C)
        coef = (rng.standard_normal((C, pr.M, 2)) * [0.2, 0.5]).astype(np.float32)
        rc, got = _call('msf', x, nf, stats, coef, -HI, HI)
        assert rc == 0
        _rows_beyond_are_zero(got, nf)
        counts = {}
        want = pr.ms_filter(x, nf, stats, coef, -HI, HI, counts=counts)
        twin = pr.ms_filter(x, nf, stats, coef, -HI, HI, np.float32)
        worst = max(worst, _worst('ms F=%d' % F, got, want, _twin_bound(want, twin)))
        if F > 1:
            assert np.abs(want[0, :F] - x[0, :F]).max() > 1e-4        # the filter did something
        if F == 1:
            assert _same_bits(got[0, :1], x[0, :1])
        for b in range(5):
            xa, na = _alone(x, nf, b)
            rc, one = _call('msf', xa, na, stats[b:b + 1], coef, -HI, HI)
            assert rc == 0 and _same_bits(one[0, :nf[b]], got[b, :nf[b]]), 'utterance %d alone differs (F=%d)' % (b, F)
    print('MEASURED ms_filter C=%d: worst fraction of 4 x the twin\'s error: %.3f' % (C, worst))


# ------------------------------------------------------------------------------------------ exact and structural
def test_identities_are_bit_exact():
    """A table of zeros, alpha = 0, one frame and constant channels: the output is the input bit for bit (-0 included), with
    tables that would otherwise change it a lot."""
    C = 65
    x, nf = _case(97, C, 5)
    x[0, :, 7] = np.float32(0.3)                                     # constant channels, among moving ones
    x[4, :97, 64] = np.float32(0.7)
    x[0, 5, 3] = -0.0
    nf[3] = 1
    x[3, 1:] = NAN
    rc, stats = _call('stats', x, nf)
    assert rc == 0 and stats[0, 7, 0] == np.float32(0.3) and stats[0, 7, 1] == 0 and stats[4, 64, 0] == np.float32(0.7) and not stats[3, :, 1].any()
    strong = np.tile(np.array([0.3, 1.5], np.float32), (C, pr.M, 1))
    gv_t = np.full(C, 0.5, np.float32)

    def same_where(y, rows):
        for b, n in enumerate(nf):
            sel = rows(b, n)
            assert _same_bits(y[b, :n][sel], x[b, :n][sel]), b
        _rows_beyond_are_zero(y, nf)

    everything = lambda b, n: np.ones((n, C), bool)
    rc, y = _call('msf', x, nf, stats, np.zeros((C, pr.M, 2), np.float32), -HI, HI)
    assert rc == 0
    same_where(y, everything)
    rc, y = _call('gv', x, nf, stats, gv_t, 0.0, 4.0)
    assert rc == 0
    same_where(y, everything)
    const = lambda b, n: (np.arange(C)[None, :] == (7 if b == 0 else 64 if b == 4 else -1)) | np.full((n, C), b == 3)
    for kind, table, s0, s1 in (('msf', strong, -HI, HI), ('gv', gv_t, 1.0, 4.0)):
        rc, y = _call(kind, x, nf, stats, table, s0, s1)
        assert rc == 0
        same_where(y, const)
        assert np.abs(y[0, :97, 0] - x[0, :97, 0]).max() > 1e-3 and np.abs(y[4, :97, 5] - x[4, :97, 5]).max() > 1e-3
    rc, ms = _call('mss', x, nf, stats)
    assert rc == 0 and not ms[0, 7].any() and not ms[4, 64].any() and not ms[3].any() and ms[0, 0, :, 0].min() >= 3


@pytest.mark.parametrize('n', [-1, -2 ** 31, 2 ** 31 - 1, 34])
def test_counts_outside_the_row_are_clamped(n):
    """max_frames = 33: a count of -1 or -2^31 is an empty utterance, one of 2^31 - 1 or max_frames + 1 is max_frames; nothing
    outside the buffers is touched and the outputs are the clamped count's, bit for bit."""
    C, maxF = 63, 33
    x = np.stack([_traj(np.random.default_rng(50 + b), maxF, C) for b in range(2)])
    nf, clamped = [n, 20], [0 if n < 0 else maxF, 20]
    x[1, 20:] = NAN
    rc, stats = _call('stats', x, nf)
    rc2, ref = _call('stats', x, clamped)
    assert rc == 0 and rc2 == 0 and _same_bits(stats, ref)
    coef = np.tile(np.array([0.2, 0.5], np.float32), (C, pr.M, 1))
    for kind, table, s0, s1 in (('gv', np.full(C, 0.01, np.float32), 1.0, 4.0), ('msf', coef, -HI, HI), ('mss', None, 0, 0)):
        rc, y = _call(kind, x, nf, ref, table, s0, s1)
        rc2, want = _call(kind, x, clamped, ref, table, s0, s1)
        assert rc == 0 and rc2 == 0 and _same_bits(y, want), kind
        if kind != 'mss':
            _rows_beyond_are_zero(y, clamped)
            assert bool(y[0].any()) == (n > 0)


def test_both_clamps_are_reached():
    """GV: a target of 100 times (a hundredth of) the variance asks for g = 10 (0.1) and gets g_max = 4 (1 / 4): the same
    bits as a target that asks for exactly that.  MS: b = +-10 with a = 0 asks for e^+-10 and gets e^hi, e^lo: the same bits
    as b = hi, lo, and not those of half the exponent."""
    C, F = 64, 97
    x = np.stack([_traj(np.random.default_rng(60), F, C)])
    stats = pr.traj_stats(x, None, np.float32)
    var = stats[0, :, 1]
    for factor, g in ((100.0, 4.0), (0.01, 0.25)):
        rc, y = _call('gv', x, None, stats, (var * np.float32(factor)).astype(np.float32), 1.0, 4.0)
        rc2, want = _call('gv', x, None, stats, (var * np.float32(g * g)).astype(np.float32), 1.0, 1e6)
        assert rc == 0 and rc2 == 0
        dev = x[0] - stats[0, :, 0]
        assert np.abs((y[0] - stats[0, :, 0]) - g * dev).max() <= 8 * U            # exactly g_max (1 / g_max) times the deviation
        assert np.abs(y - want).max() <= 8 * U
    table = lambda b: np.tile(np.array([0.0, b], np.float32), (C, pr.M, 1))
    for b, lim in ((10.0, HI), (-10.0, -HI)):
        rc, y = _call('msf', x, None, stats, table(b), -HI, HI)
        rc2, want = _call('msf', x, None, stats, table(lim), -HI, HI)
        rc3, half = _call('msf', x, None, stats, table(0.5 * lim), -HI, HI)
        assert rc == 0 and rc2 == 0 and rc3 == 0 and _same_bits(y, want) and np.abs(y - half).max() > 1e-3
        ref = pr.ms_filter(x, None, stats, table(b), -HI, HI)
        _worst('ms clamp %g' % b, y, ref, _twin_bound(ref, pr.ms_filter(x, None, stats, table(b), -HI, HI, np.float32)))


def test_bins_at_the_floor_get_gain_one():
    """Deviations of 1e-12 about 0: |X|^2 <= (64 * 1e-12)^2 < 1e-20 in every bin, so nothing is counted and the strongest
    table returns the input bit for bit; the same trajectories ten thousand times larger are above the floor and change."""
    C, F = 80, 70
    rng = np.random.default_rng(70)
    x = (1e-12 * rng.uniform(-1.0, 1.0, (1, F, C))).astype(np.float32)
    strong = np.tile(np.array([0.0, 2.0], np.float32), (C, pr.M, 1))
    for scale, passes in ((1.0, True), (10000.0, False)):
        xs = (x * np.float32(scale)).astype(np.float32)
        stats = pr.traj_stats(xs, None, np.float32)
        rc, y = _call('msf', xs, None, stats, strong, -HI, HI)
        rc2, ms = _call('mss', xs, None, stats)
        assert rc == 0 and rc2 == 0
        assert _same_bits(y, xs) == passes and bool(ms.any()) == (not passes)
        if not passes:
            assert ms[0, :, 1:, 0].min() >= 1 and np.abs(y - xs).max() > 1e-10


def test_refusals_leave_the_outputs_untouched():
    C, F = 5, 9
    x = np.stack([_traj(np.random.default_rng(80), F, C)] * 2)
    stats = pr.traj_stats(x, None, np.float32)
    gv_t, coef = np.full(C, 0.01, np.float32), np.zeros((C, pr.M, 2), np.float32)
    args = {'stats': dict(), 'gv': dict(stats=stats, table=gv_t, s0=1.0, s1=4.0), 'mss': dict(stats=stats),
            'msf': dict(stats=stats, table=coef, s0=-HI, s1=HI)}
    ptr_names = {'stats': ('x', 'out'), 'gv': ('x', 'stats', 'table', 'out'), 'mss': ('x', 'stats', 'out'), 'msf': ('x', 'stats', 'table', 'out')}
    n_refused = 0

    def refused(code, kind, **kw):
        nonlocal n_refused
        rc, out = _call(kind, x, [F, 4], **dict(args[kind], **kw))
        assert rc == code and np.isnan(out).all(), (kind, kw, rc)
        n_refused += 1

    for kind in args:
        for name in ptr_names[kind]:
            refused(1, kind, null=name)
        for shape in ((0, F, C), (2, 0, C), (2, F, 0), (2, -3, C)):
            refused(1, kind, shape=shape)
        for shape in ((65536, F, C), (2, 16385, C), (2, F, 2050)):
            refused(4, kind, shape=shape)
    for kw in (dict(s0=-0.5), dict(s0=1.01), dict(s0=NAN), dict(s1=0.99), dict(s1=float('inf')), dict(alias=True)):
        refused(1, 'gv', **kw)
    for kw in (dict(s0=0.5), dict(s1=-0.5), dict(s0=float('-inf')), dict(s1=NAN), dict(alias=True)):
        refused(1, 'msf', **kw)
    assert n_refused == 13 + 16 + 12 + 11


# ------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_of_the_four_launches():
    """All four captured once (after the warm-up call _capture makes), replayed with other trajectories, counts and tables
    copied into the static tensors: bit-identical to eager calls on the same inputs."""
    import postfilter
    from test_graph_replay_gpu import _capture, _free, _same
    B, F, C = 3, 70, 201

    def inputs(k):
        rng = np.random.default_rng(90 + k)
        x = np.stack([_traj(rng, F, C) for _ in range(B)])
        nf = np.array([F - 3 * k, 33 + k, 0 if k == 1 else 5], np.int32)
        coef = (rng.standard_normal((C, pr.M, 2)) * [0.2, 0.5]).astype(np.float32)
        gv_t = rng.uniform(0.001, 0.01, C).astype(np.float32)
        return [torch.from_numpy(a).cuda() for a in (x, nf, coef, gv_t)]

    def chain(x, nf, coef, gv_t):
        st = postfilter.traj_stats_batch(x, nf)
        ms = postfilter.ms_stats_batch(x, nf, st)
        y = postfilter.ms_filter_batch(x, nf, st, coef, -HI, HI)
        z = postfilter.gv_filter_batch(y, nf, postfilter.traj_stats_batch(y, nf), gv_t, 1.0, 4.0)
        return st, ms, y, z

    static = inputs(0)
    g, outs = _capture(lambda: chain(*static))
    try:
        for k in range(1, 3):
            new = inputs(k)
            for s, t in zip(static, new):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            want = chain(*new)
            for name, a, b in zip(('stats', 'ms', 'y', 'z'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert torch.isfinite(outs[3]).all() and float((outs[3][0] - new[0][0]).abs().max()) > 1e-4
    finally:
        _free(g)


# ------------------------------------------------------------------------------------------ convert_postfilter_batch
@pytest.fixture(scope='module')
def plain_run(f32_models):
    """convert_batch on the toy models, the model fitted on its own true and predicted spectra, and the tables."""
    import conversion
    import postfilter
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    plain = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, phase='device', seed=5)
    model = postfilter.fit([(plain.stft_true, plain.n_frames)], [(plain.stft_pred, plain.n_frames)])
    return plain, model, postfilter.upload(model, 0.85)


def test_convert_postfilter_batch_is_the_separate_calls(f32_models, plain_run):
    import conversion
    import postfilter
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    plain, model, tables = plain_run
    wav, lens = _ragged()
    assert model.gv_t.shape == (201,) and np.isfinite(postfilter.ms_coef(model, 0.85)).all()
    r = conversion.convert_postfilter_batch(dec, wav, lens, c, model=model, mode='ms+gv', n_iter=N_ITER, seed=5)
    assert r.n_frames == plain.n_frames and r.n_samples == plain.n_samples and r.y_wav_true is None
    for name in ('mel_true', 'mel_pred', 'stft_true', 'phn_pred'):
        assert torch.equal(getattr(r, name), getattr(plain, name)), name
    assert torch.equal(r.stft_raw, plain.stft_pred)
    d_nf = torch.tensor(plain.n_frames, dtype=torch.int32, device='cuda')
    y = postfilter.ms_filter_batch(plain.stft_pred, d_nf, postfilter.traj_stats_batch(plain.stft_pred, d_nf), tables.coef, -HI, HI)
    z = postfilter.gv_filter_batch(y, d_nf, postfilter.traj_stats_batch(y, d_nf), tables.gv_t, 1.0, 4.0)
    assert torch.equal(r.stft_pred, z) and float((z - plain.stft_pred).abs().max()) > 1e-4
    d_ids = torch.arange(3, dtype=torch.int32, device='cuda')
    _, wave = conversion._vocoder_tail(c, d_nf, d_ids, N_ITER, 0.0, 1.0, 5, 'device', 'device', None, z, None)
    assert torch.equal(r.y_wav_pred, wave) and torch.isfinite(wave).all() and not torch.equal(wave, plain.y_wav_pred)
    for b, n in enumerate(r.n_frames):
        assert not r.stft_pred[b, n:].any()
    one = conversion.convert_postfilter_batch(dec, wav, lens, c, model=tables, mode='ms', n_iter=N_ITER, seed=5)
    assert torch.equal(one.stft_pred, y)
    with pytest.raises(ValueError, match='model'):
        conversion.convert_postfilter_batch(dec, wav, lens, c)
    with pytest.raises(ValueError, match='mode'):
        conversion.convert_postfilter_batch(dec, wav, lens, c, model=model, mode='sm')


def test_convert_postfilter_batch_at_strength_zero_is_convert_batch(f32_models, plain_run):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    plain, model, _ = plain_run
    wav, lens = _ragged()
    r = conversion.convert_postfilter_batch(dec, wav, lens, c, model=model, mode='ms+gv', k=0.0, alpha=0.0, n_iter=N_ITER, seed=5)
    assert torch.equal(r.stft_pred, plain.stft_pred) and torch.equal(r.stft_raw, plain.stft_pred)
    assert torch.equal(r.y_wav_pred, plain.y_wav_pred)


def test_convert_postfilter_batch_no_host_synchronisation(f32_models, plain_run):
    """bf16 models, cuda inputs, the model's tables uploaded beforehand, warmed up: under torch's sync debug mode 'error' any
    device-to-host copy, blocking upload or host wait inside the call raises."""
    import conversion
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    dec32, wd, enc_cfg, dec_cfg, c = f32_models
    _, _, tables = plain_run
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(dict(enc_cfg, compute_dtype='bfloat16'), None)
        dec = decoder_specs(dict(dec_cfg, compute_dtype='bfloat16'), None, enc)
    dec.store.load_dict(dict(wd), strict=False)
    wav, lens = _ragged()
    d_wav = torch.from_numpy(wav).cuda()
    calls = (dict(mode='ms'), dict(mode='gv'), dict(mode='ms+gv', realse=1.2, out_sr=22050))
    for kw in calls:                                                # warm-up
        conversion.convert_postfilter_batch(dec, d_wav, lens, c, model=tables, n_iter=N_ITER, window_batch=4, **kw)
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        rs = [conversion.convert_postfilter_batch(dec, d_wav, lens, c, model=tables, n_iter=N_ITER, window_batch=4, **kw) for kw in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.y_wav_pred).all() and float(r.y_wav_pred.abs().max()) > 0 for r in rs)
    assert not torch.equal(rs[0].stft_pred, rs[1].stft_pred) and torch.equal(rs[0].stft_raw, rs[1].stft_raw)
