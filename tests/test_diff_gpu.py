"""Differential-spectrum conversion on the MI355X: the gain launch and the filter launch alone through the C ABI against
tests/diff_ref.py (float64, and for the gain its float32 twin), graph replay of both, and conversion.convert_diff_batch.

Every kernel call as tests/test_vocoder_kernels_gpu.py makes them: every buffer inside sentinel bands that are checked after
the call, workspace and outputs filled with NaN, gain rows at or beyond an utterance's frame count NaN, waveform samples at
or beyond its length NaN, out_stride = L + 37."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import diff_ref as dr
import vocoder_kernels_cases as vc
import vocoder_kernels_ref as vr
from test_convert_batch_gpu import _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)

pytestmark = pytest.mark.gpu

BAND = 1024
SENT = np.float32(-98765.4375)
NAN = float('nan')
SLACK = 37
FILTER_CASES = ('ship', 'n16', 'n64-hop64', 'skew16')


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


def _measured(what, got, want, bound):
    """One MEASURED line for the element with the worst error / bound; an element whose bound is 0 must be exact.  No element
    is left out."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape and got.size > 0
    assert np.isfinite(got).all(), what + ': the device value is not finite'
    err = np.abs(got - want)
    zero = bound <= 0.0
    assert not err[zero].any(), what + ': an element with bound 0 is not exact'
    if zero.all():
        print('MEASURED %s: error 0 bound 0 ratio 0.000 (all exact)' % what)
        return 0.0
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print('MEASURED %s: error %.3e bound %.3e ratio %.3f' % (what, err[i], bound[i], ratio[i]))
    assert ratio[i] <= 1.0, '%s: error %.3e > bound %.3e at %s' % (what, err[i], bound[i], i)
    return float(ratio[i])


# ------------------------------------------------------------------------------------------ the gain launch
def _gain_call(pred, tru, nf, norm, alpha, boost, cut, taps, null=None, n_taps=None):
    """One vc_spectral_diff_gain_f32 call on guarded buffers: (rc, gain [B, F, nb] as the device left it, NaN where unwritten)."""
    import _vc
    lib = _vc.lib()
    B, F, nb = pred.shape
    d_p, d_t, d_c = Guarded(pred.size, host=pred), Guarded(tru.size, host=tru), Guarded(len(taps), host=taps)
    d_g = Guarded(pred.size, fill=NAN)
    d_nf = None if nf is None else torch.tensor(list(nf), dtype=torch.int32, device='cuda')
    ptrs = dict(pred=_vc.ptr(d_p.t), tru=_vc.ptr(d_t.t), taps=_vc.ptr(d_c.t), gain=_vc.ptr(d_g.t))
    if null:
        ptrs[null] = None
    rc = lib.vc_spectral_diff_gain_f32(ptrs['pred'], ptrs['tru'], _vc.ptr(d_nf), B, F, nb, float(norm), float(alpha), float(boost),
                                       float(cut), ptrs['taps'], len(taps) if n_taps is None else n_taps, ptrs['gain'],
                                       _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_p, 'd_pred'), (d_t, 'd_true'), (d_c, 'd_taps'), (d_g, 'd_gain')):
        g.check(what)
    assert _same_bits(d_p.numpy(), pred.reshape(-1)) and _same_bits(d_t.numpy(), tru.reshape(-1)), 'an input was written'
    return rc, d_g.numpy().reshape(B, F, nb)


def _poison_rows(a, nf):
    a = a.copy()
    for b, n in enumerate(nf):
        a[b, min(max(n, 0), a.shape[1]):] = NAN
    return a


def test_gain_exact_grid():
    """P_dB_norm_factor = 2^-6, both spectra integer multiples of it, taps 1/4 1/2 1/4: every difference is an integer, every
    product and partial sum a multiple of 1/4 below 2^7 -- s has one value whatever the order of the sum.  G is exactly 1.0
    wherever s == 0, sits at both clamps where s does, and equals exp2 of the twin's exponent within the exponential's bound
    everywhere."""
    rng = np.random.RandomState(1)
    B, F, nb = 2, 17, 201
    q = 2.0 ** -6
    pred = (rng.randint(-8, 65, (B, F, nb)) * q).astype(np.float32)
    tru = (rng.randint(-8, 65, (B, F, nb)) * q).astype(np.float32)
    tru[0, 3] = pred[0, 3]                                        # a row of s == 0
    pred[0, 4], tru[0, 4] = 1.0, 0.0                              # +64 dB: the boost clamp
    pred[0, 5], tru[0, 5] = -0.25, 1.0                            # -64 dB (the negative input counts as 0): the cut clamp
    pred[1, 0, :40], tru[1, 0, :40] = 0.5, 0.5                    # a stretch of zeros next to random bins
    nf = [F, 9]
    taps = np.array([0.25, 0.5, 0.25], np.float32)
    for alpha in (1.0, 0.5):
        rc, G = _gain_call(_poison_rows(pred, nf), _poison_rows(tru, nf), nf, q, alpha, 20.0, 30.0, taps)
        assert rc == 0
        s64 = dr.gain_s(pred, tru, nf, q, taps, alpha, 20.0, 30.0)
        s32 = dr.gain_s(pred, tru, nf, q, taps, alpha, 20.0, 30.0, dtype=np.float32)
        ok = ~np.isnan(s64)
        assert np.array_equal(s32[ok].astype(np.float64), s64[ok])                       # the grid is exact in float32
        assert (G[ok][s64[ok] == 0.0] == 1.0).all() and (s64[ok] == 0.0).sum() >= 201 + 38
        assert (s64[0, 4] == 20.0).all() and (s64[0, 5] == -30.0).all() and (s64[ok] == 20.0).sum() >= 201 and (s64[ok] == -30.0).sum() >= 201
        hi, lo = G[ok][s64[ok] == 20.0], G[ok][s64[ok] == -30.0]
        assert len(set(_bits(hi).tolist())) == 1 and len(set(_bits(lo).tolist())) == 1
        want = dr.gain_from_s(s32)
        _measured('gain grid alpha=%g' % alpha, G[ok], want[ok], dr.exp2_rel_bound() * want[ok])
        assert abs(float(hi[0]) - 10.0) <= 10.0 * dr.exp2_rel_bound() + 10.0 * 2 * 20 * dr.U * np.log(10.0) / 20.0
        for b, n in enumerate(nf):
            assert not G[b, n:].any() and not np.isnan(G[b]).any()


@pytest.mark.parametrize('n_taps', [1, 3, 17, 65])
@pytest.mark.parametrize('nb', [201, 9, 33])
def test_gain_random(nb, n_taps):
    """Random spectra (negative values included: they count as 0) at F = 1, 15, 16, 17, 33 in a ragged batch with one empty
    utterance: G against float64 within the derived relative bound, against exp2 of the float32 twin's exponent within the
    exponential's bound alone (so the clamped s is the twin's, bit for bit, up to what the exponential can hide), rows at or
    beyond n_frames exactly 0."""
    taps = dr.smoothing_taps((n_taps - 1) // 2)
    norm = 0.01
    for F in (1, 15, 16, 17, 33):
        rng = np.random.RandomState(1000 * nb + 10 * n_taps + F)
        nf = [F, 0, max(F // 2, 1), F - 1]
        pred = rng.uniform(-0.1, 0.9, (4, F, nb)).astype(np.float32)
        tru = rng.uniform(-0.1, 0.9, (4, F, nb)).astype(np.float32)
        rc, G = _gain_call(_poison_rows(pred, nf), _poison_rows(tru, nf), nf, norm, 1.0, 20.0, 30.0, taps)
        assert rc == 0
        s64 = dr.gain_s(pred, tru, nf, norm, taps, 1.0, 20.0, 30.0)
        ok = ~np.isnan(s64)
        g64 = dr.gain_from_s(s64)
        rel = dr.gain_rel_bound(pred, tru, nf, norm, taps, 1.0)
        tag = 'nb=%d taps=%d F=%d' % (nb, n_taps, F)
        _measured('gain vs float64 ' + tag, G[ok], g64[ok], (rel * g64)[ok])
        g32 = dr.gain_from_s(dr.gain_s(pred, tru, nf, norm, taps, 1.0, 20.0, 30.0, dtype=np.float32))
        _measured('gain vs twin ' + tag, G[ok], g32[ok], dr.exp2_rel_bound() * g32[ok])
        assert not G[~ok].any() and not np.isnan(G).any()
        assert F < 16 or (pred[ok] < 0).any()
    # n_frames == NULL: every row
    rc, G = _gain_call(pred, tru, None, norm, 1.0, 20.0, 30.0, taps)
    g32 = dr.gain_from_s(dr.gain_s(pred, tru, None, norm, taps, 1.0, 20.0, 30.0, dtype=np.float32))
    assert rc == 0
    _measured('gain vs twin, all rows nb=%d taps=%d' % (nb, n_taps), G, g32, dr.exp2_rel_bound() * g32)


def test_gain_batch_through_python_and_alpha_zero():
    import conversion
    rng = np.random.RandomState(3)
    pred, tru = (rng.uniform(-0.1, 0.9, (3, 20, 201)).astype(np.float32) for _ in range(2))
    nf = [20, 7, 0]
    G = conversion.diff_gain_batch(pred, tru, nf, 0.01).cpu().numpy()
    g32 = dr.gain_from_s(dr.gain_s(pred, tru, nf, 0.01, dr.smoothing_taps(8), 1.0, 20.0, 30.0, dtype=np.float32))
    _measured('diff_gain_batch', G, g32, dr.exp2_rel_bound() * g32)
    d_nf = torch.tensor(nf, dtype=torch.int32, device='cuda')
    G0 = conversion.diff_gain_batch(torch.from_numpy(pred).cuda(), torch.from_numpy(tru).cuda(), d_nf, 0.01, alpha=0.0).cpu().numpy()
    assert (G0[0] == 1.0).all() and (G0[1, :7] == 1.0).all() and not G0[1, 7:].any() and not G0[2].any()


def test_gain_refusals_launch_nothing():
    import _vc
    pred, tru = np.zeros((1, 4, 201), np.float32), np.zeros((1, 4, 201), np.float32)
    taps = dr.smoothing_taps(8)
    base = dict(norm=0.01, alpha=1.0, boost=20.0, cut=30.0)
    bad = [dict(null='pred'), dict(null='tru'), dict(null='taps'), dict(null='gain'), dict(n_taps=16), dict(n_taps=67), dict(n_taps=0),
           dict(alpha=1.5), dict(alpha=-0.5), dict(alpha=NAN), dict(boost=-1.0), dict(cut=-1.0), dict(boost=float('inf')), dict(cut=NAN),
           dict(norm=0.0), dict(norm=NAN)]
    for kw in bad:
        a = dict(base, **{k: v for k, v in kw.items() if k in base})
        rc, G = _gain_call(pred, tru, [4], a['norm'], a['alpha'], a['boost'], a['cut'], np.resize(taps, 67) if kw.get('n_taps') == 67 else taps,
                           null=kw.get('null'), n_taps=kw.get('n_taps'))
        assert rc == 1 and b'vc_spectral_diff_gain_f32' in _vc.lib().vc_last_error(), kw
        assert kw.get('null') == 'gain' or np.isnan(G).all(), kw
    rc, G = _gain_call(pred, tru, [4], **base, taps=taps)
    assert rc == 0 and (G == 1.0).all()


# ------------------------------------------------------------------------------------------ the filter launch
_PLANS = {}


def _plan(cid):
    import _vc
    if cid not in _PLANS:
        n_fft, win, hop, _ = vc.geometry(cid)
        taps = vc.taps(cid)
        h = C.c_void_p()
        _vc.check(_vc.lib().vc_vocoder_plan_create(win, hop, n_fft, _vc.ptr(taps), C.byref(h)))
        _PLANS[cid] = (h, taps)
    return _PLANS[cid][0]


@pytest.fixture(scope='module', autouse=True)
def _plans_destroyed_at_the_end():
    yield
    import _vc
    torch.cuda.synchronize()
    for h, _ in _PLANS.values():
        _vc.lib().vc_vocoder_plan_destroy(h)
    _PLANS.clear()


def _ws_bytes(n_fft, B, maxF):
    return vr.align256(B * maxF * n_fft * 4) + vr.align256(4 * B)


class Result:
    pass


def _filter_call(cid, wav, lens, G, nf, out_stride=None, ws_short=0, null=None, expect_ok=True):
    """One vc_stft_filter_f32 call.  wav [B, wav_stride] float32 (NaN at or beyond an utterance's length already), lens as
    given to the device, G [B, maxF, bins] float32, nf list or None."""
    import _vc
    lib = _vc.lib()
    n_fft, win, hop, _ = vc.geometry(cid)
    B, maxF, nb = G.shape
    assert nb == 1 + n_fft // 2
    L = hop * (maxF - 1)
    stride = L + SLACK if out_stride is None else out_stride
    total = lib.vc_stft_filter_workspace_bytes(_plan(cid), B, maxF)
    assert total == _ws_bytes(n_fft, B, maxF)
    d_x, d_G = Guarded(wav.size, host=wav), Guarded(G.size, host=G)
    d_y = Guarded(B * max(stride, 1), fill=NAN)
    d_ws = Guarded(total // 4 + 4, fill=NAN)
    d_len = torch.tensor(list(lens), dtype=torch.int32, device='cuda')
    d_nf = None if nf is None else torch.tensor(list(nf), dtype=torch.int32, device='cuda')
    p = dict(plan=_plan(cid), wav=_vc.ptr(d_x.t), len=_vc.ptr(d_len), gain=_vc.ptr(d_G.t), out=_vc.ptr(d_y.t), ws=_vc.ptr(d_ws.t))
    if null:
        p[null] = None
    rc = lib.vc_stft_filter_f32(p['plan'], p['wav'], wav.shape[1], p['len'], p['gain'], _vc.ptr(d_nf), B, maxF, p['out'], stride,
                                p['ws'], total - ws_short, _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_x, 'd_wav'), (d_G, 'd_gain'), (d_y, 'd_out'), (d_ws, 'the workspace')):
        g.check(what)
    assert _same_bits(d_x.numpy(), wav.reshape(-1)) and _same_bits(d_G.numpy(), G.reshape(-1)), 'an input was written'
    r = Result()
    r.rc, r.err = rc, (lib.vc_last_error() or b'') if rc else b''
    r.out_raw, r.ws_raw = d_y.numpy(), d_ws.numpy()
    if not expect_ok:
        return r
    _vc.check(rc)
    r.out = r.out_raw.reshape(B, stride)
    fb = vr.align256(B * maxF * n_fft * 4)
    r.frames = r.ws_raw[:B * maxF * n_fft].reshape(B, maxF, n_fft)
    r.F = r.ws_raw[fb // 4:fb // 4 + B].view(np.int32)
    assert np.isnan(r.ws_raw[fb // 4 + B:]).all() and np.isnan(r.ws_raw[B * maxF * n_fft:fb // 4]).all()
    want_F = [dr.frames_used(min(max(int(n), 0), wav.shape[1]), None if nf is None else nf[b], maxF, n_fft, hop) for b, n in enumerate(lens)]
    assert r.F.tolist() == want_F, (r.F.tolist(), want_F)
    for b, F in enumerate(want_F):
        assert np.isnan(r.frames[b, F:]).all(), 'a frame row beyond F_b was written'
        assert not r.out[b, max(hop * (F - 1), 0):].any(), 'output beyond hop (F_b - 1) is not zero'
    return r


def _signals(cid, specs, seed, wav_stride=None):
    """Noise utterances for (F, r) pairs: len = hop (F - 1) + r.  Returns (wav [B, stride] with NaN from len on, lens)."""
    n_fft, win, hop, _ = vc.geometry(cid)
    lens = [hop * (F - 1) + r for F, r in specs]
    stride = (max(lens) + 5) if wav_stride is None else wav_stride
    rng = np.random.RandomState(seed)
    wav = np.full((len(lens), stride), NAN, np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = 0.1 * rng.standard_normal(n)
    return wav, lens


def _gains(kind, B, maxF, nb, Fs, seed):
    rng = np.random.RandomState(seed)
    G = np.full((B, maxF, nb), NAN, np.float32)
    for b, F in enumerate(Fs):
        G[b, :F] = rng.uniform(0.1, 4.0, (F, nb)) if kind == 'random' else {'one': 1.0, 'half': 0.5}[kind]
    return G


def _check_against_float64(tag, cid, r, wav, lens, G):
    n_fft, win, hop, _ = vc.geometry(cid)
    w = vc.window(cid)
    worst = 0.0
    for b, F in enumerate(r.F.tolist()):
        if F == 0:
            assert not r.out[b].any()
            continue
        x = wav[b, :lens[b]].astype(np.float64)
        want, bound = dr.filter_bound(x, G[b, :F].astype(np.float64), w, hop, n_use=F)
        worst = max(worst, _measured('%s %s utt %d (F %d, len %d)' % (tag, cid, b, F, lens[b]), r.out[b, :hop * (F - 1)], want, bound))
    return worst


def _reconstructible(cid, F):
    """Samples of the trimmed output where the window sum-square exceeds float32 tiny (elsewhere istft leaves the sum as it is)."""
    n_fft, win, hop, _ = vc.geometry(cid)
    w = vc.window(cid)
    wss = np.zeros(n_fft + hop * (F - 1))
    for f in range(F):
        wss[f * hop:f * hop + n_fft] += w * w
    return vr.trim(wss, n_fft) > vr.F32_TINY


@pytest.mark.parametrize('F', ['min', 15, 16, 17, 33])
@pytest.mark.parametrize('cid', FILTER_CASES)
def test_filter_lengths_and_gains(cid, F):
    """len = hop (F - 1) + r for r = 0, 1, hop - 1 as one batch, d_n_frames NULL.  G == 1 returns the input, G == 0.5 half of
    it, a random G in [0.1, 4] on noise the float64 filter -- each within the bound derived in tests/diff_ref.py."""
    n_fft, win, hop, _ = vc.geometry(cid)
    F = vr.min_frames(n_fft, hop) if F == 'min' else F
    specs = [(F, 0), (F, 1), (F, hop - 1)]
    wav, lens = _signals(cid, specs, seed=F)
    for kind in ('one', 'half', 'random'):
        G = _gains(kind, 3, F, 1 + n_fft // 2, [F] * 3, seed=F + 1)
        r = _filter_call(cid, wav, lens, G, None)
        assert r.F.tolist() == [F] * 3
        _check_against_float64('filter G=' + kind, cid, r, wav, lens, G)
        if kind != 'random':
            c = 1.0 if kind == 'one' else 0.5
            ok = _reconstructible(cid, F)
            for b in range(3):
                x = wav[b, :hop * (F - 1)].astype(np.float64)
                ref = dr.stft_filter(wav[b, :lens[b]].astype(np.float64), G[b, :F].astype(np.float64), vc.window(cid), hop)
                assert np.abs(ref - c * x)[ok].max() <= 1e-12 * np.abs(x).max()          # in float64 the pass IS c * x
                _, bound = dr.filter_bound(wav[b, :lens[b]].astype(np.float64), G[b, :F].astype(np.float64), vc.window(cid), hop)
                assert (np.abs(r.out[b, :hop * (F - 1)] - c * x)[ok] <= bound[ok] + 1e-12 * np.abs(x).max()).all()


@pytest.mark.parametrize('cid', FILTER_CASES)
def test_filter_ragged_batch_cut_and_alone(cid):
    """A ragged batch of 3 (33, 17 and the fewest frames), once with d_n_frames NULL and once with counts that cut the first
    utterance short of 1 + len / hop (the cut at t_e), ask for more than the second has and leave the third; then every
    utterance again alone under another batch size, max_frames and out_stride: bit-identical."""
    n_fft, win, hop, _ = vc.geometry(cid)
    Fmin = vr.min_frames(n_fft, hop)
    specs = [(33, 1), (17, hop - 1), (Fmin, 0)]
    wav, lens = _signals(cid, specs, seed=5)
    nb = 1 + n_fft // 2
    for nf in (None, [21, 29, Fmin]):
        Fs = [33, 17, Fmin] if nf is None else [21, 17, Fmin]
        G = _gains('random', 3, 33, nb, Fs, seed=6)
        r = _filter_call(cid, wav, lens, G, nf)
        assert r.F.tolist() == Fs
        _check_against_float64('ragged nf=%s' % (nf,), cid, r, wav, lens, G)
        for b, F in enumerate(Fs):
            Ga = np.full((1, F + 2, nb), NAN, np.float32)
            Ga[0, :F] = G[b, :F]
            a = _filter_call(cid, wav[b:b + 1, :lens[b] + 1].copy(), [lens[b]], Ga, None if nf is None else [nf[b]], out_stride=hop * (F + 1) + 11)
            assert a.F.tolist() == [F]
            assert _same_bits(a.out[0, :hop * (F - 1)], r.out[b, :hop * (F - 1)]) and _same_bits(a.frames[0, :F], r.frames[b, :F])


@pytest.mark.parametrize('cid', ('ship', 'n16'))
def test_filter_short_and_junk_lengths(cid):
    """len <= N / 2 and hop (F - 1) <= N / 2 give zero rows; lengths of 0, -1 and 2^31 - 1 (clamped to wav_stride: the whole row
    is then the signal) write nothing outside their rows; the good utterance between them does not notice."""
    n_fft, win, hop, _ = vc.geometry(cid)
    half = n_fft // 2
    Fmin = vr.min_frames(n_fft, hop)
    F = Fmin + 9
    stride = hop * (F - 1) + 3
    wav, _ = _signals(cid, [(F, 3)] * 7, seed=9, wav_stride=stride)
    lens = [half, hop * (Fmin - 2) + hop - 1, 0, -1, 2 ** 31 - 1, stride - 1, -2 ** 31]
    for b, n in enumerate(lens):
        wav[b, min(max(n, 0), stride):] = NAN
    nb = 1 + n_fft // 2
    Fs = [dr.frames_used(min(max(n, 0), stride), None, F, n_fft, hop) for n in lens]
    assert Fs[:4] == [0, 0, 0, 0] and Fs[4] == F and Fs[5] == F and Fs[6] == 0 and lens[1] > half
    G = _gains('random', 7, F, nb, Fs, seed=10)
    r = _filter_call(cid, wav, lens, G, None)
    eff = [min(max(n, 0), stride) for n in lens]
    _check_against_float64('junk lengths', cid, r, wav, eff, G)
    for b in (0, 1, 2, 3, 6):
        assert not r.out[b].any()
    a = _filter_call(cid, wav[5:6].copy(), [lens[5]], G[5:6].copy(), None)
    assert _same_bits(a.out, r.out[5:6])
    # counts that are junk: negative, and far above max_frames
    r2 = _filter_call(cid, wav[4:6].copy(), [stride, stride - 1], G[4:6].copy(), [-5, 2 ** 31 - 1])
    assert r2.F.tolist() == [0, F] and _same_bits(r2.out[1], r.out[5])


@pytest.mark.parametrize('cid', ('ship', 'n16'))
def test_filter_refusals_launch_nothing(cid):
    import _vc
    n_fft, win, hop, _ = vc.geometry(cid)
    F = vr.min_frames(n_fft, hop) + 3
    wav, lens = _signals(cid, [(F, 1)], seed=2)
    G = _gains('one', 1, F, 1 + n_fft // 2, [F], seed=0)
    bad = [(dict(null=k), 1) for k in ('plan', 'wav', 'len', 'gain', 'out', 'ws')] + [(dict(out_stride=hop * (F - 1) - 1), 1), (dict(ws_short=1), 3)]
    for kw, code in bad:
        r = _filter_call(cid, wav, lens, G, None, expect_ok=False, **kw)
        assert r.rc == code and b'vc_stft_filter_f32' in r.err, (kw, r.rc, r.err)
        assert np.isnan(r.out_raw).all() and np.isnan(r.ws_raw).all(), kw
    lib = _vc.lib()
    assert lib.vc_stft_filter_workspace_bytes(_plan(cid), 0, 5) == 0 and lib.vc_stft_filter_workspace_bytes(_plan(cid), 2, 0) == 0
    assert lib.vc_stft_filter_workspace_bytes(_plan(cid), 3, 129) == vr.align256(3 * 129 * n_fft * 4) + 256
    assert lib.vc_stft_filter_workspace_bytes(_plan(cid), 65, 2) == vr.align256(65 * 2 * n_fft * 4) + 512
    good = _filter_call(cid, wav, lens, G, None)
    assert good.rc == 0 and good.F.tolist() == [F]


def test_stft_filter_batch_through_python():
    import audio_lib
    wav, lens = _signals('ship', [(33, 1), (17, 79), (4, 0)], seed=12)
    G = _gains('random', 3, 33, 201, [33, 17, 4], seed=13)
    raw = _filter_call('ship', wav, lens, G, None)
    y = audio_lib.stft_filter_batch(np.nan_to_num(wav), lens, np.nan_to_num(G))
    assert tuple(y.shape) == (3, 80 * 32) and _same_bits(y.cpu().numpy(), raw.out[:, :80 * 32])
    d_len = torch.tensor(lens, dtype=torch.int32, device='cuda')
    d_nf = torch.tensor([20, 17, 4], dtype=torch.int32, device='cuda')
    y2 = audio_lib.stft_filter_batch(torch.from_numpy(np.nan_to_num(wav)).cuda(), d_len, torch.from_numpy(np.nan_to_num(G)).cuda(), d_nf)
    cut = _filter_call('ship', wav, lens, G, [20, 17, 4])
    assert _same_bits(y2.cpu().numpy(), cut.out[:, :80 * 32]) and not y2[0, 80 * 19:].any()


# ------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_of_gain_and_filter():
    """Both calls captured once (after the warm-up call _capture makes), replayed with other spectra, waveforms, lengths and
    frame counts copied into the static tensors: bit-identical to eager calls on the same inputs."""
    import audio_lib
    import conversion
    from test_graph_replay_gpu import _capture, _free, _same
    B, F, Lmax = 3, 40, 80 * 39 + 60
    plan = audio_lib._get_voc_plan(400, 80, 400)
    d_taps = torch.from_numpy(dr.smoothing_taps(8)).cuda()

    def inputs(k):
        rng = np.random.RandomState(20 + k)
        lens = np.array([Lmax - 13 * k, 80 * (20 + k) + 7, 150 + 50 * k], np.int32)
        nf = np.array([40 - k, 40, 5], np.int32)
        return [torch.from_numpy(rng.uniform(-0.1, 0.9, (B, F, 201)).astype(np.float32)).cuda(),
                torch.from_numpy(rng.uniform(-0.1, 0.9, (B, F, 201)).astype(np.float32)).cuda(),
                torch.from_numpy((0.1 * rng.standard_normal((B, Lmax))).astype(np.float32)).cuda(),
                torch.from_numpy(lens).cuda(), torch.from_numpy(nf).cuda()]

    def chain(pred, tru, wav, lens, nf):
        g = conversion._diff_gain_launch(pred, tru, nf, 0.01, 1.0, 20.0, 30.0, d_taps)
        return g, audio_lib._stft_filter_launch(plan, wav, lens, g, nf)

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
            for name, a, b in zip(('gain', 'y'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert float(outs[1][0].abs().max()) > 0 and torch.isfinite(outs[1]).all()
            assert bool(outs[1][2].any()) == (k == 2)                       # 200 samples at k = 1: not more than the reflect padding
    finally:
        _free(g)


# ------------------------------------------------------------------------------------------ convert_diff_batch
def _normalise(y, d_nf, c):
    import audio_lib
    import _vc
    y = y.clone()
    vplan = audio_lib._get_voc_plan(c['win_length'], c['hop_length'], c['n_fft'])
    _vc.check(_vc.lib().vc_inv_preemphasis_normalize(vplan.handle, _vc.ptr(y), _vc.ptr(d_nf), y.shape[0], 1 + y.shape[1] // c['hop_length'],
                                                     y.shape[1], 0.0, float(15 * c['mean_abs_amp_norm']), _vc.current_stream()))
    return y


def test_convert_diff_batch_is_the_separate_calls(f32_models):
    import audio_lib
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    hop = c['hop_length']
    r = conversion.convert_diff_batch(dec, wav, lens, c)
    plain = conversion.convert_batch(dec, wav, lens, c, vocode=False)
    n_use, n_samples = conversion.diff_frames(conversion.convert_plan(lens, c, 0, 60, True), hop)
    assert r.n_frames == n_use.tolist() == [641, 301, 1001] and r.n_samples == n_samples.tolist() and r.f0_src is None
    for name in ('mel_true', 'mel_pred', 'stft_true', 'stft_pred', 'phn_pred'):
        assert torch.equal(getattr(r, name), getattr(plain, name)), name
    d_nf = torch.tensor(n_use.tolist(), dtype=torch.int32, device='cuda')
    gain = conversion.diff_gain_batch(plain.stft_pred, plain.stft_true, d_nf, c['P_dB_norm_factor'])
    assert torch.equal(r.gain, gain)
    y = audio_lib.stft_filter_batch(wav, lens, gain, d_nf, c['win_length'], hop, c['n_fft'])
    assert torch.equal(r.y_wav_pred, _normalise(y, d_nf, c)) and tuple(y.shape) == (3, hop * 1199)
    out = r.y_wav_pred.cpu().numpy()
    for b, n in enumerate(r.n_samples):
        assert np.isfinite(out[b]).all() and not out[b, n:].any() and out[b, :n].any()
        _measured('level utt %d' % b, float(np.abs(out[b, :n].astype(np.float64)).mean()), 0.045, (vr.block_sum_terms(n) + 8 + 2) * vr.U * 0.045)
    g = r.gain.cpu().numpy()
    for b, n in enumerate(r.n_frames):                               # inside the clamps where there is a gain, 0 elsewhere
        assert g[b, :n].min() >= 10.0 ** -1.5 * (1 - 1e-6) and g[b, :n].max() <= 10.0 * (1 + 1e-6) and not g[b, n:].any()


def test_convert_diff_batch_alpha_zero_returns_the_source(f32_models):
    """alpha = 0: G == 1, so the output is the source span at the output level, within the filter's bound pushed through the
    level launch's (vocoder_kernels_ref.normalize_bound)."""
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_diff_batch(dec, wav, lens, c, alpha=0.0)
    w = vr.device_window(vr.padded_window(400, 400))
    out = r.y_wav_pred.cpu().numpy()
    for b, (F, n) in enumerate(zip(r.n_frames, r.n_samples)):
        assert bool((r.gain[b, :F] == 1.0).all())
        x = wav[b, :lens[b]].astype(np.float64)
        y, yb = dr.filter_bound(x, np.ones((F, 201)), w, 80, n_use=F)
        assert np.abs(y - x[:n]).max() <= 1e-12
        want, bound = vr.normalize(x[:n], 0.045), vr.normalize_bound(y, yb, 0.045)
        _measured('alpha 0 utt %d' % b, out[b, :n], want, bound)


def test_convert_diff_batch_no_host_synchronisation(f32_models):
    """cuda inputs, warmed up: under torch's sync debug mode 'error' any device-to-host copy, blocking upload or host wait
    inside the call raises.  A ratio, the source's own contour mapped between two speakers' statistics, a contour, and both
    resamplers."""
    import conversion
    import evaluation
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    d_wav = torch.from_numpy(wav).cuda()
    f_in = evaluation.f0_track_batch(wav, lens)
    st_src = conversion.f0_stats_batch(f_in.f0, torch.tensor(f_in.n_frames, dtype=torch.int32, device='cuda'))
    st_tgt = conversion._F0_STATS_NT(st_src.count, st_src.mean + 0.2, st_src.std * 1.1)
    contour = torch.zeros((3, 1200), device='cuda')                  # Hz per frame of the output grid; 0: leave the frame
    contour[:, :f_in.f0.shape[1]] = f_in.f0 * 1.1
    calls = (dict(), dict(pitch=1.2), dict(pitch='source', stats_src=st_src, stats_tgt=st_tgt), dict(pitch=contour),
             dict(wav_sr=8000, out_sr=22050, lens=[n // 2 for n in lens]))
    for kw in calls:                                                # warm-up
        conversion.convert_diff_batch(dec, d_wav, **dict(dict(lens=lens, cfg_d=c, window_batch=4), **kw))
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        rs = [conversion.convert_diff_batch(dec, d_wav, **dict(dict(lens=lens, cfg_d=c, window_batch=4), **kw)) for kw in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.y_wav_pred).all() and float(r.y_wav_pred.abs().max()) > 0 for r in rs)
    assert torch.equal(rs[1].f0_src, f_in.f0) and torch.equal(rs[2].f0_src, f_in.f0) and rs[0].f0_src is None
    assert not torch.equal(rs[1].y_wav_pred, rs[0].y_wav_pred) and torch.equal(rs[1].gain, rs[0].gain)
    # the shifted source is what the filter saw: the separate calls on it give the same bits
    import audio_lib
    sh = conversion.pitch_shift_batch(d_wav, lens, f_in.f0, 16000, 80, ratio=1.2)
    d_nf = torch.tensor(rs[1].n_frames, dtype=torch.int32, device='cuda')
    y = audio_lib.stft_filter_batch(sh.y, lens, rs[1].gain, d_nf)
    assert torch.equal(rs[1].y_wav_pred, _normalise(y, d_nf, c))
    # both resamplers: the lengths at 16 kHz give the plan, its n_samples go out at 22.05 kHz
    l16 = audio_lib.resample_len(np.array(calls[4]['lens']), 8000, 16000)
    _, ns16 = conversion.diff_frames(conversion.convert_plan(l16, c, 0, 60, True), 80)
    assert rs[4].n_samples == [int(v) for v in audio_lib.resample_len(ns16, 16000, 22050)]
    assert all(not rs[4].y_wav_pred[b, n:].any() for b, n in enumerate(rs[4].n_samples))


@pytest.mark.parametrize('kind', ['bfloat16', 'mxfp8'])
def test_low_precision_decoders_through_convert_diff_batch(f32_models, kind):
    """A bf16 decoder, and an MX-FP8 decoder built without an encoder and fed through encoder=: runs, finite, at the level."""
    import conversion
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    dec32, wd, enc_cfg, dec_cfg, c = f32_models
    enc_cfg = dict(enc_cfg, compute_dtype='bfloat16')
    dec_cfg = dict(dec_cfg, compute_dtype=kind)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
        dec = decoder_specs(dec_cfg, None, enc if kind == 'bfloat16' else None)
        if kind == 'mxfp8':
            enc.restore()
    dec.store.load_dict(dict(wd), strict=False)
    wav, lens = _ragged()
    r = conversion.convert_diff_batch(dec, wav, lens, c, encoder=enc if kind == 'mxfp8' else None)
    assert torch.isfinite(r.y_wav_pred).all() and torch.isfinite(r.gain).all() and r.n_frames == [641, 301, 1001]
    out = r.y_wav_pred.cpu().numpy()
    for b, n in enumerate(r.n_samples):
        assert abs(float(np.abs(out[b, :n]).mean()) - 0.045) <= 1e-5 and not out[b, n:].any()
    if kind == 'mxfp8':
        with pytest.raises(ValueError, match='encoder'):
            conversion.convert_diff_batch(dec, wav, lens, c)
