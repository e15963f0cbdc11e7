"""Noise suppression on the MI355X: vc_stft_power_f32 and vc_noise_gain_f32 alone through the C ABI against
tests/denoise_ref.py (float64, and for the gain its float32 twin), identity alone / in a batch / under graph replay,
enhance.denoise_batch end to end and denoise= of the conversion entry points.

Every kernel call as tests/test_diff_gpu.py makes them: every buffer inside sentinel bands that are checked after the call,
outputs filled with NaN, power rows at or beyond an utterance's frame count NaN, waveform samples at or beyond its length NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import denoise_cases as dc
import denoise_ref as dr
import vocoder_kernels_cases as vc
import vocoder_kernels_ref as vr
from test_convert_batch_gpu import _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)
from test_denoise_cpu import FLOOR_DB, HOP, LEAD, SR, W, closed_form_gain, vowel_case

pytestmark = pytest.mark.gpu

BAND = 1024
SENT = np.float32(-98765.4375)
NAN = float('nan')
POWER_CASES = ('ship', 'n16', 'n64-hop64', 'skew16')


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
    """One MEASURED line for the element with the worst error / bound; an element whose bound is 0 must be exact."""
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


def _dev_i32(v):
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device='cuda')


# ------------------------------------------------------------------------------------------ the power launch
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


def _power_call(cid, wav, lens, nf, maxF, null=None, batch=None, max_frames=None, stride=None):
    """One vc_stft_power_f32 call on guarded buffers: (rc, power [B, maxF, nb] as the device left it, frame counts as int32
    bit patterns of the NaN-filled buffer)."""
    import _vc
    lib = _vc.lib()
    n_fft = vc.geometry(cid)[0]
    B, nb = wav.shape[0], 1 + n_fft // 2
    d_x, d_P, d_F = Guarded(wav.size, host=wav), Guarded(B * maxF * nb, fill=NAN), Guarded(B, fill=NAN)
    d_len, d_nf = _dev_i32(lens), _dev_i32(nf)
    p = dict(plan=_plan(cid), wav=_vc.ptr(d_x.t), len=_vc.ptr(d_len), power=_vc.ptr(d_P.t), fout=_vc.ptr(d_F.t))
    if null:
        p[null] = None
    rc = lib.vc_stft_power_f32(p['plan'], p['wav'], wav.shape[1] if stride is None else stride, p['len'], _vc.ptr(d_nf),
                               B if batch is None else batch, maxF if max_frames is None else max_frames, p['power'], p['fout'],
                               _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_x, 'd_wav'), (d_P, 'd_power'), (d_F, 'd_frames_out')):
        g.check(what)
    assert _same_bits(d_x.numpy(), wav.reshape(-1)), 'the waveform was written'
    return rc, d_P.numpy().reshape(B, maxF, nb), d_F.numpy().view(np.int32)


def _power_batch(cid, seed=5):
    """Three utterances: an exact multiple of hop over a tile plus one frame, a partial last tile with a remainder, and one
    of exactly n_fft / 2 samples (the reflect padding does not fit: a zero row).  NaN from each length on."""
    n_fft, win, hop, frames = vc.geometry(cid)
    Fa, Fb = frames[1], frames[2]
    lens = [hop * (Fa - 1), hop * (Fb - 1) + max(hop // 2, 1) - (1 if hop > 2 else 0), n_fft // 2]
    rng = np.random.RandomState(seed)
    wav = np.full((3, max(lens) + 5), NAN, np.float32)
    for b, n in enumerate(lens):
        wav[b, :n] = 0.1 * rng.standard_normal(n)
    return wav, lens, Fa, Fb


def _check_power(tag, cid, wav, lens, nf, maxF, P, Fout):
    n_fft, win, hop, _ = vc.geometry(cid)
    w = vc.window(cid)
    for b, n in enumerate(lens):
        n = min(max(int(n), 0), wav.shape[1])
        want, F, bound = dr.power(wav[b].astype(np.float64), n, None if nf is None else nf[b], maxF, w, hop)
        assert int(Fout[b]) == F, (tag, b, int(Fout[b]), F)
        assert not P[b, F:].any() and not np.isnan(P[b]).any(), '%s utt %d: a row at or beyond F_b is not 0' % (tag, b)
        if F:
            _measured('power %s %s utt %d (F %d, len %d)' % (cid, tag, b, F, n), P[b, :F], want[:F], bound[:F])


@pytest.mark.parametrize('cid', POWER_CASES)
def test_power_ragged_batch_against_float64(cid):
    """B = 3 with a zero row (len <= n_fft / 2) and a length that is an exact multiple of hop; frame counts below, equal to
    and above 1 + len / hop, negative, and NULL; one more row than any utterance has frames.  Against float64 with the bound
    of tests/denoise_ref.py: power's float32 model, the forward half's of tests/vocoder_kernels_ref.py; the frame counts the
    device reports are exact; the inputs are unwritten."""
    n_fft, win, hop, _ = vc.geometry(cid)
    wav, lens, Fa, Fb = _power_batch(cid)
    full = [1 + n // hop for n in lens]
    maxF = max(full) + 1
    lo = vr.min_frames(n_fft, hop)
    assert lo < full[0] and lo < full[1]
    for tag, nf in (('null', None), ('below-equal', [full[0] - 1, full[1], 5]), ('above-negative', [full[0] + 3, -2, 0]),
                    ('smallest-one', [lo, lo - 1, maxF])):
        rc, P, Fout = _power_call(cid, wav, lens, nf, maxF)
        assert rc == 0
        _check_power(tag, cid, wav, lens, nf, maxF, P, Fout)
    # junk lengths are clamped to [0, wav_stride] on the device: the row beyond the longest utterance stays NaN-free input
    junk = np.where(np.isnan(wav), np.float32(0.05), wav)
    rc, P, Fout = _power_call(cid, junk, [-7, 10 ** 9, lens[2] + 1], None, maxF)
    assert rc == 0
    _check_power('junk-lens', cid, junk, [-7, 10 ** 9, lens[2] + 1], None, maxF, P, Fout)


@pytest.mark.parametrize('cid', ('ship', 'n16'))
def test_power_refusals_launch_nothing(cid):
    import _vc
    wav, lens, _, _ = _power_batch(cid)
    maxF = 1 + max(lens) // vc.geometry(cid)[2]
    for kw in (dict(null='plan'), dict(null='wav'), dict(null='len'), dict(null='power'), dict(null='fout'), dict(batch=0),
               dict(batch=65536), dict(max_frames=0), dict(stride=0)):
        rc, P, Fout = _power_call(cid, wav, lens, None, maxF, **kw)
        assert rc == 1 and b'vc_stft_power_f32' in _vc.lib().vc_last_error(), kw
        assert np.isnan(P).all() and (Fout == np.float32(NAN).view(np.int32)).all(), kw


def test_stft_power_batch_through_python_is_the_filters_framing():
    """audio_lib.stft_power_batch equals the C call, and its frame counts are the filter's own (read back from the filter's
    workspace by tests/test_diff_gpu.py; here: the unit-gain filter returns hop (F - 1) samples of the input)."""
    import audio_lib
    wav, lens, _, _ = _power_batch('ship')
    clean = np.nan_to_num(wav)
    nf = [10, 37, 7]
    P, d_F = audio_lib.stft_power_batch(clean, lens, nf)
    maxF = 1 + wav.shape[1] // 80
    rc, want, Fout = _power_call('ship', wav, lens, nf, maxF)
    assert tuple(P.shape) == (3, maxF, 201) and _same_bits(P.cpu().numpy(), want) and d_F.cpu().tolist() == Fout.tolist() == [10, 37, 0]
    y = audio_lib.stft_filter_batch(clean, lens, torch.ones_like(P), d_F).cpu().numpy()
    for b, F in enumerate(Fout):
        n = 80 * max(F - 1, 0)
        assert not y[b, n:].any() and (F == 0 or np.abs(y[b, :n] - clean[b, :n]).max() < 1e-5)


# ------------------------------------------------------------------------------------------ the gain launch
def _cfg(c):
    import _vc
    return _vc.DenoiseCfg(int(c['rule']), int(c['n_init']), c['a_spp'], c['a_noise'], c['a_dd'], c['xi_h1'], c['xi_min'], c['gain_min'],
                          c['gamma_max'])


def _poison_rows(a, nf):
    a = np.array(a, np.float32)
    for b, n in enumerate(nf):
        a[b, min(max(n, 0), a.shape[1]):] = NAN
    return a


def _gain_call(P, nf, noise0, cfg, want_noise=True, null=None, shape=None):
    """One vc_noise_gain_f32 call on guarded buffers: (rc, gain, noise or None), NaN where the device wrote nothing.  Rows of
    P at or beyond an utterance's count hold NaN."""
    import _vc
    lib = _vc.lib()
    B, maxF, nb = P.shape
    host = P if nf is None else _poison_rows(P, nf)
    d_P, d_G = Guarded(P.size, host=host), Guarded(P.size, fill=NAN)
    d_S = Guarded(P.size, fill=NAN) if want_noise else None
    d_0 = None if noise0 is None else Guarded(noise0.size, host=noise0)
    c = cfg if isinstance(cfg, C.Structure) else _cfg(cfg)
    p = dict(power=_vc.ptr(d_P.t), gain=_vc.ptr(d_G.t), cfg=C.byref(c))
    if null:
        p[null] = None
    B_, maxF_, nb_ = shape or (B, maxF, nb)
    rc = lib.vc_noise_gain_f32(p['power'], _vc.ptr(_dev_i32(nf)), None if d_0 is None else _vc.ptr(d_0.t), B_, maxF_, nb_, p['cfg'],
                               p['gain'], None if d_S is None else _vc.ptr(d_S.t), _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_P, 'd_power'), (d_G, 'd_gain'), (d_S, 'd_noise'), (d_0, 'd_noise0')):
        if g is not None:
            g.check(what)
    assert _same_bits(d_P.numpy(), host.reshape(-1)) and (d_0 is None or _same_bits(d_0.numpy(), noise0.reshape(-1))), 'an input was written'
    return rc, d_G.numpy().reshape(P.shape), None if d_S is None else d_S.numpy().reshape(P.shape)


def _rows_beyond_are_zero(counts, *outs):
    for a in outs:
        assert not np.isnan(a).any(), 'an element was not written'
        for b, n in enumerate(counts):
            assert not a[b, min(max(n, 0), a.shape[1]):].any(), 'a row at or beyond the frame count is not 0'


@pytest.mark.parametrize('nb', (65, 201))
def test_gain_without_transcendentals_is_the_twin_bit_for_bit(nb):
    """Rule 0, a_dd == 0, a_noise == 1, noise0 given: nothing the exponentials produce reaches the gain, so the device, the
    float32 twin and the closed form agree in every bit; the noise track is noise0 in every live row."""
    P, counts, noise0 = dc.inputs(nb, 'long')
    cfg = dr.config(rule=0, a_dd=0.0, a_noise=1.0)
    rc, G, S = _gain_call(P, counts, noise0, cfg)
    assert rc == 0
    _rows_beyond_are_zero(counts, G, S)
    twin, s32 = dr.noise_gain(P, counts, noise0, cfg, dtype=np.float32)
    assert _same_bits(G, twin) and _same_bits(G, closed_form_gain(P, counts, noise0, cfg)) and _same_bits(S, s32)
    assert len(np.unique(G)) > 1000


@pytest.mark.parametrize('rule', (0, 1))
def test_gain_freeze_is_bit_identical(rule):
    P, counts, noise0 = dc.inputs(65, 'long')
    noise0 = noise0.copy()
    noise0[0, :4] = 0.0                                              # raised to FLT_MIN once, then frozen there
    rc, G, S = _gain_call(P, counts, noise0, dr.config(rule=rule, a_noise=1.0))
    assert rc == 0
    _rows_beyond_are_zero(counts, G, S)
    for b, n in enumerate(np.clip(counts, 0, P.shape[1])):
        assert _same_bits(S[b, :n], np.broadcast_to(np.maximum(noise0[b], np.float32(dr.FLT_MIN)), (n, 65)))
    assert np.isfinite(G).all() and G[0, :300].min() >= np.float32(0.1) and G.max() <= 1.0


@pytest.mark.parametrize('with_noise0', (False, True))
@pytest.mark.parametrize('rule', (0, 1))
def test_gain_scales_exactly_by_powers_of_two(rule, with_noise0):
    """P and noise0 times 2^m, m = +-20: the gain keeps every bit and the noise track is scaled exactly."""
    P, counts, noise0 = dc.inputs(201, 'long')
    n0 = noise0 if with_noise0 else None
    cfg = dr.config(rule=rule)
    rc, G, S = _gain_call(P, counts, n0, cfg)
    assert rc == 0 and S.max() > 0
    for m in (-20, 20):
        k = np.float32(2.0 ** m)
        rc, G2, S2 = _gain_call(P * k, counts, None if n0 is None else n0 * k, cfg)
        assert rc == 0 and _same_bits(G2, G) and _same_bits(S2, S * k), m


@pytest.mark.parametrize('rule', (0, 1))
def test_gain_of_all_zero_power_is_finite(rule):
    P = np.zeros((2, 20, 65), np.float32)
    for n0 in (None, np.zeros((2, 65), np.float32)):
        rc, G, S = _gain_call(P, [20, 11], n0, dr.config(rule=rule))
        assert rc == 0 and np.isfinite(G).all() and np.isfinite(S).all()
        _rows_beyond_are_zero([20, 11], G, S)
        assert (G[0] >= np.float32(0.1)).all() and (G[0] <= 1.0).all() and (S[0] == np.float32(dr.FLT_MIN)).all()


@pytest.mark.parametrize('rule', (0, 1))
@pytest.mark.parametrize('nb', dc.NBINS)
def test_gain_general_against_float64(nb, rule):
    """tests/denoise_cases.py: B = 4 (two noisy vowels, two of exponential noise), frame counts 1, n_init - 1, n_init,
    n_init + 1, 70, 300, 0 and one above max_frames, with and without noise0.  Against float64 with the bound 4 x the float32
    twin's own largest distance from float64 on the case (absolute for the gain, relative for the noise power); a lane whose
    float64 pb comes within 1e-5 of the 0.99 guard is left out from that frame on (at most 5 % of the lanes:
    tests/test_denoise_cpu.py).  Also: the call without d_noise gives the same gain."""
    for kind in dc.LAUNCHES:
        maxF, counts = dc.LAUNCHES[kind]
        for with_noise0 in (False, True):
            P, _, noise0 = dc.inputs(nb, kind)
            g64, s64, left_out, bound_g, bound_s = dc.reference(nb, rule, kind, with_noise0)
            cfg = dr.config(rule=rule, n_init=dc.N_INIT)
            rc, G, S = _gain_call(P, counts, noise0 if with_noise0 else None, cfg)
            assert rc == 0
            _rows_beyond_are_zero(counts, G, S)
            tag = 'nb=%d rule=%d %s noise0=%d' % (nb, rule, kind, with_noise0)
            keep = ~left_out
            assert dc.lanes_left_out(left_out, counts) <= 0.05
            _measured('gain ' + tag, G[keep], g64[keep], bound_g)
            live = keep & (s64 > 0.0)
            _measured('noise ' + tag, S[live] / s64[live], np.ones(int(live.sum())), bound_s)
            assert (G[s64 > 0.0] >= np.float32(0.1)).all() and G.max() <= 1.0
            if kind == 'short':
                rc, G1, S1 = _gain_call(P, counts, noise0 if with_noise0 else None, cfg, want_noise=False)
                assert rc == 0 and S1 is None and _same_bits(G1, G)


def test_gain_null_counts_and_refusals():
    import _vc
    P, counts, noise0 = dc.inputs(33, 'short')
    cfg = dr.config()
    rc, G, S = _gain_call(P, None, None, cfg)
    rc2, G2, S2 = _gain_call(P, [P.shape[1]] * 4, None, cfg)
    assert rc == 0 and rc2 == 0 and _same_bits(G, G2) and _same_bits(S, S2) and not np.isnan(G).any()
    neg = [-3, P.shape[1] + 40, 0, 5]                                # a negative count counts as 0, one above max_frames as max_frames
    rc, G3, S3 = _gain_call(P, neg, None, cfg)
    assert rc == 0 and not G3[0].any() and not S3[0].any() and not G3[2].any()
    _rows_beyond_are_zero(neg, G3, S3)
    assert _same_bits(G3[1], G[1]) and _same_bits(S3[1], S[1]) and G3[3, :5].min() >= np.float32(0.1)
    bad = [dict(null='power'), dict(null='gain'), dict(null='cfg'), dict(shape=(0, 9, 33)), dict(shape=(65536, 9, 33)),
           dict(shape=(4, 0, 33)), dict(shape=(4, 9, 1)), dict(shape=(4, 9, 2050))]
    bad += [dict(cfg=dr.config(**kw)) for kw in (dict(rule=2), dict(rule=-1), dict(n_init=0), dict(a_spp=1.5), dict(a_spp=-0.5),
                                                  dict(a_dd=1.5), dict(a_dd=float('nan')), dict(a_noise=0.0), dict(a_noise=1.5),
                                                  dict(xi_h1=0.0), dict(xi_h1=float('inf')), dict(xi_min=-1.0), dict(xi_min=float('nan')),
                                                  dict(gamma_max=0.0), dict(gamma_max=float('inf')), dict(gain_min=0.0),
                                                  dict(gain_min=1.5))]
    for kw in bad:
        rc, G, S = _gain_call(P, counts, None, kw.pop('cfg', cfg), **kw)
        assert rc == 1 and b'vc_noise_gain_f32' in _vc.lib().vc_last_error(), kw
        assert np.isnan(G).all() and np.isnan(S).all(), kw


# ------------------------------------------------------------------------------------------ identity
def _noisy(hz, snr_db, seed, seconds=1.0):
    clean, noise = dr.noisy_vowel(hz, snr_db, seed, seconds=seconds, lead=0.3)
    return (clean + noise).astype(np.float32)


def test_each_launch_alone_equals_in_a_batch_of_four():
    import audio_lib
    import enhance
    xs = [_noisy(120.0, 10, 1), _noisy(210.0, 0, 2, 0.7), _noisy(150.0, 20, 3, 0.4), _noisy(90.0, 5, 4, 0.9)]
    lens = [len(x) for x in xs]
    wav = np.zeros((4, max(lens)), np.float32)
    for b, x in enumerate(xs):
        wav[b, :lens[b]] = x
    plan = audio_lib._get_voc_plan(400, HOP, 400)
    cfg = enhance.gain_cfg('t')
    d_wav, d_len = torch.from_numpy(wav).cuda(), _dev_i32(lens)
    Fmax = 1 + wav.shape[1] // HOP
    r = enhance._denoise_launch(plan, d_wav, d_len, None, Fmax, cfg, None, True)
    P, _ = audio_lib._stft_power_launch(plan, d_wav, d_len, None, Fmax)
    assert r.n_frames.cpu().tolist() == [1 + n // HOP for n in lens]
    for b in range(4):
        one = enhance._denoise_launch(plan, d_wav[b:b + 1].contiguous(), d_len[b:b + 1].contiguous(), None, Fmax, cfg, None, True)
        P1, F1 = audio_lib._stft_power_launch(plan, d_wav[b:b + 1].contiguous(), d_len[b:b + 1].contiguous(), None, Fmax)
        assert torch.equal(P1[0], P[b]) and int(F1[0]) == int(r.n_frames[b])
        for name in ('y', 'gain', 'noise'):
            assert torch.equal(getattr(one, name)[0], getattr(r, name)[b]), (b, name)
    assert torch.isfinite(r.y).all() and float(r.y.abs().max()) > 0


def test_graph_replay_of_the_three_launches():
    """power, gain, filter captured once, replayed with other waveforms and lengths copied into the static tensors:
    bit-identical to eager calls on the same inputs."""
    import audio_lib
    import enhance
    from test_graph_replay_gpu import _capture, _free, _same
    B, Lmax = 3, HOP * 99 + 41
    plan = audio_lib._get_voc_plan(400, HOP, 400)
    cfg = enhance.gain_cfg('t', rule='logmmse')
    Fmax = 1 + Lmax // HOP

    def inputs(k):
        rng = np.random.RandomState(30 + k)
        lens = np.array([Lmax - 17 * k, HOP * (40 + 9 * k), 150 + 60 * k], np.int32)
        return [torch.from_numpy((0.1 * rng.standard_normal((B, Lmax))).astype(np.float32)).cuda(), torch.from_numpy(lens).cuda()]

    def chain(wav, lens):
        r = enhance._denoise_launch(plan, wav, lens, None, Fmax, cfg, None, True)
        return r.y, r.gain, r.noise, r.n_frames

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
            for name, a, b in zip(('y', 'gain', 'noise', 'n_frames'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert outs[3].cpu().tolist() == [1 + (Lmax - 17 * k) // HOP, 41 + 9 * k, 0 if k == 1 else 4]
            assert float(outs[0][0].abs().max()) > 0 and torch.isfinite(outs[0]).all()
    finally:
        _free(g)


# ------------------------------------------------------------------------------------------ end to end
def test_denoise_batch_on_the_noisy_vowel():
    """The 10 dB vowels of tests/test_denoise_cpu.py through enhance.denoise_batch: output SNR (of the device's waveform),
    final noise level and lead attenuation equal the float64 restatement's to the 0.1 dB they are quoted at; the
    mel-cepstral distortion to the clean vowel falls."""
    import enhance
    import evaluation
    from test_convert_batch_cpu import CFG
    cases = [(120.0, 10), (210.0, 10)]
    sig = [dr.noisy_vowel(hz, snr, seed=int(hz) + snr, lead=LEAD) for hz, snr in cases]
    x = np.stack([(c + n).astype(np.float32) for c, n in sig])
    n = x.shape[1]
    r = enhance.denoise_batch(x, [n, n], sr=SR, return_noise=True)
    F = 1 + n // HOP
    assert tuple(r.y.shape) == (2, HOP * (F - 1)) and r.n_frames.cpu().tolist() == [F, F] and tuple(r.gain.shape) == (2, F, 201)
    y, G, S = r.y.cpu().numpy(), r.gain.cpu().numpy(), r.noise.cpu().numpy()
    cfg = dr.config()
    for b, ((hz, snr), (clean, noise)) in enumerate(zip(cases, sig)):
        want = vowel_case(hz, snr)
        P, _, _ = dr.power(x[b].astype(np.float64), n, None, F, W, HOP)
        psd = dr.true_psd(noise, W)
        _, snr_out = dr.snr_figures(clean, noise, G[b], W, HOP, int(LEAD * SR), y=y[b])
        att, expected, bias = dr.lead_figures(P, G[b], S[b], psd, int(LEAD * SR) // HOP, cfg)
        psd_err = dr.psd_error_db(S[b], F, psd)
        print('MEASURED denoise_batch %g Hz at %d dB: SNR out %.3f (float64 %.3f), noise level %+.3f (%+.3f), lead attenuation %.3f (%.3f), '
              'floor %g dB' % (hz, snr, snr_out, want[1], psd_err, want[2], att, want[3], FLOOR_DB))
        assert abs(snr_out - want[1]) <= 0.1 and abs(psd_err - want[2]) <= 0.1 and abs(att - want[3]) <= 0.1
        assert snr_out > want[0]
    clean = np.stack([c.astype(np.float32) for c, _ in sig])[:, :HOP * (F - 1)]
    L = [HOP * (F - 1)] * 2
    before = evaluation.mcd_wav_batch(np.ascontiguousarray(x[:, :L[0]]), L, np.ascontiguousarray(clean), L, CFG)
    after = evaluation.mcd_wav_batch(r.y, L, np.ascontiguousarray(clean), L, CFG)
    m0, m1 = (v.total / v.path_len for v in (before, after))
    print('MEASURED mel-cepstral distortion to the clean vowel: noisy %s dB, denoised %s dB' % (m0.cpu().tolist(), m1.cpu().tolist()))
    assert bool((m1 < m0).all())


def test_convert_batch_without_denoise_is_unchanged(f32_models):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    a = conversion.convert_batch(dec, wav, lens, c, n_iter=2)
    for dn in (None, False):
        b = conversion.convert_batch(dec, wav, lens, c, n_iter=2, denoise=dn)
        for name in a._fields:
            u, v = getattr(a, name), getattr(b, name)
            assert (torch.equal(u, v) if torch.is_tensor(u) else u == v), name


def test_convert_entry_points_with_denoise(f32_models):
    """convert_batch(denoise=True) and convert_diff_batch(denoise=True) are the same calls on the denoised input cut to whole
    hops -- bit for bit, so everything those calls promise (lengths, zeros beyond them) holds -- and the stage they add,
    conversion._denoise_input, replays in a graph."""
    import conversion
    import enhance
    from test_graph_replay_gpu import _capture, _free, _same
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    rng = np.random.RandomState(4)
    lens = [lens[0] - 33, lens[1], lens[2] - 79]                     # two lengths that are no multiple of the hop
    wav = (wav + 0.01 * rng.standard_normal(wav.shape)).astype(np.float32)
    hop = c['hop_length']
    cut = [hop * (n // hop) for n in lens]
    for kw in (True, dict(rule='wiener', floor_db=12.0)):
        opts = {} if kw is True else kw
        dn = enhance.denoise_batch(wav, cut, sr=c['sample_rate'], win_length=c['win_length'], hop_length=hop, n_fft=c['n_fft'], **opts)
        assert dn.n_frames.cpu().tolist() == [1 + n // hop for n in cut]
        for b, n in enumerate(cut):
            assert not bool(dn.y[b, n:].any())
        r = conversion.convert_batch(dec, wav, lens, c, n_iter=2, denoise=kw)
        want = conversion.convert_batch(dec, dn.y, cut, c, n_iter=2)
        assert r.n_frames == want.n_frames and r.n_samples == want.n_samples == [hop * (f - 1) for f in r.n_frames]
        for name in ('y_wav_pred', 'mel_true', 'stft_true', 'mel_pred', 'stft_pred', 'phn_pred'):
            assert torch.equal(getattr(r, name), getattr(want, name)), name
        assert torch.isfinite(r.y_wav_pred).all() and tuple(r.y_wav_pred.shape) == (3, hop * (max(r.n_frames) - 1))
        for b, n in enumerate(r.n_samples):
            assert bool(r.y_wav_pred[b, :n].any()) and not bool(r.y_wav_pred[b, n:].any())
        d = conversion.convert_diff_batch(dec, wav, lens, c, denoise=kw)
        dwant = conversion.convert_diff_batch(dec, dn.y, cut, c)
        assert d.n_frames == dwant.n_frames and d.n_samples == dwant.n_samples == [hop * (f - 1) for f in d.n_frames]
        for name in ('y_wav_pred', 'gain', 'stft_true', 'stft_pred'):
            assert torch.equal(getattr(d, name), getattr(dwant, name)), name
        assert torch.isfinite(d.y_wav_pred).all()
        for b, n in enumerate(d.n_samples):
            assert bool(d.y_wav_pred[b, :n].any()) and not bool(d.y_wav_pred[b, n:].any())
    plain = conversion.convert_batch(dec, wav, lens, c, vocode=False)
    assert not torch.equal(plain.stft_true, want.stft_true)

    # ---- the added stage under graph replay
    h = conversion._convert_host('t', dec, wav, lens, c, 0, 60, True, None, 64, True, None, None, None, 'kaiser_best', denoise=True)
    up = conversion._convert_upload(h, wav, [])
    torch.cuda.synchronize()
    g, out = _capture(lambda: conversion._denoise_input(h, up, c, h.denoise)[1].wav)
    try:
        g.replay()
        torch.cuda.synchronize()
        eager = enhance.denoise_batch(wav, cut, sr=c['sample_rate'], win_length=c['win_length'], hop_length=hop, n_fft=c['n_fft']).y
        _same(out, eager, 'the captured stage')
        up.wav.copy_(torch.flip(up.wav, [0]))
        up.d_lens.copy_(torch.flip(up.d_lens, [0]))
        g.replay()
        torch.cuda.synchronize()
        flipped = enhance.denoise_batch(wav[::-1].copy(), cut[::-1], sr=c['sample_rate'], win_length=c['win_length'], hop_length=hop,
                                        n_fft=c['n_fft']).y
        _same(out, flipped, 'the replayed stage')
    finally:
        _free(g)
