"""Differential-spectrum conversion on the host (tests/diff_ref.py; include/vc_hip.h, "Differential-spectrum conversion"):
the restated stft / istft against tests/vocoder_kernels_ref.py, the filter's algebra, the gain's float32 twin against its
float64 definition, the taps, the method's own check on two synthetic vowels, and convert_diff_batch's host side.  No GPU."""
import numpy as np
import pytest

import diff_ref as dr
import f0_ref
import vocoder_kernels_ref as vr
from test_convert_batch_cpu import CFG

HOP, N = 80, 400
W = vr.device_window(vr.padded_window(400, 400))


def _noise(n, seed=0):
    return np.random.RandomState(seed).standard_normal(n)


# ------------------------------------------------------------------------------------------ stft, istft, the filter
@pytest.mark.parametrize('n_fft,win,hop', [(400, 400, 80), (16, 12, 5), (64, 64, 64)])
def test_restated_transforms_equal_the_vocoder_reference(n_fft, win, hop):
    w = vr.device_window(vr.padded_window(win, n_fft))
    x = _noise(hop * 9 + 3, n_fft)
    S = dr.stft(x, w, hop)
    assert S.shape == (1 + len(x) // hop, 1 + n_fft // 2)
    assert np.abs(S - vr.stft_wave(x, w, hop)).max() <= 1e-12 * np.abs(S).max()
    fr = dr.synthesis_frames(S, w)
    assert np.abs(fr - vr.frames_from_spectrum(S, w)).max() <= 1e-12 * np.abs(fr).max()
    assert np.abs(dr.istft_frames(fr, w, hop) - vr.waveform(fr, w, hop)).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize('r', [0, 1, HOP - 1])
@pytest.mark.parametrize('F', [4, 17])
def test_unit_gain_is_the_identity(F, r):
    x = _noise(HOP * (F - 1) + r, F + r)
    y = dr.stft_filter(x, np.ones((F, 201)), W, HOP)
    assert y.shape == (HOP * (F - 1),)
    e = np.abs(y - x[:len(y)]).max() / np.abs(x).max()
    print('identity F=%d r=%d: %.2e of peak' % (F, r, e))
    assert e <= 1e-12


def test_filter_is_linear_and_a_constant_gain_scales():
    F = 12
    x1, x2 = _noise(HOP * (F - 1) + 7, 1), _noise(HOP * (F - 1) + 7, 2)
    G = np.random.RandomState(3).uniform(0.1, 4.0, (F, 201))
    f = lambda x: dr.stft_filter(x, G, W, HOP)
    assert np.abs(f(2.0 * x1 - 3.0 * x2) - (2.0 * f(x1) - 3.0 * f(x2))).max() <= 1e-12 * np.abs(f(x1)).max()
    y = dr.stft_filter(x1, np.full((F, 201), 0.5), W, HOP)
    assert np.abs(y - 0.5 * x1[:len(y)]).max() <= 1e-12
    # n_use cuts the frames, not the padding: the first frames do not change, the padding stays at the signal's own end
    cut = dr.stft(x1, W, HOP, n_use=7)
    assert np.array_equal(cut, dr.stft(x1, W, HOP)[:7])


def test_frames_used():
    assert dr.frames_used(1000, None, 50, 400, 80) == 13 and dr.frames_used(1000, 9, 50, 400, 80) == 9
    assert dr.frames_used(1000, 30, 10, 400, 80) == 10 and dr.frames_used(1000, -4, 50, 400, 80) == 0
    assert dr.frames_used(200, None, 50, 400, 80) == 0 and dr.frames_used(201, None, 50, 400, 80) == 0      # 3 frames: 160 samples
    assert dr.frames_used(240, None, 50, 400, 80) == 4 and dr.frames_used(240, 3, 50, 400, 80) == 0
    assert dr.frames_used(-1, None, 50, 400, 80) == 0 and dr.frames_used(2 ** 31 - 1, 50, 50, 400, 80) == 50


# ------------------------------------------------------------------------------------------ the gain
def _spectra(B, F, nb, seed):
    rng = np.random.RandomState(seed)
    return rng.uniform(-0.1, 0.9, (B, F, nb)).astype(np.float32), rng.uniform(-0.1, 0.9, (B, F, nb)).astype(np.float32)


@pytest.mark.parametrize('h', [0, 1, 8, 32])
@pytest.mark.parametrize('nb', [201, 9])
def test_gain_float32_twin_against_float64(nb, h):
    pred, tru = _spectra(2, 5, nb, nb + h)
    taps = dr.smoothing_taps(h)
    s64 = dr.gain_s(pred, tru, [5, 3], 0.01, taps, 1.0, 20.0, 30.0)
    s32 = dr.gain_s(pred, tru, [5, 3], 0.01, taps, 1.0, 20.0, 30.0, dtype=np.float32)
    assert s32.dtype == np.float32 and np.isnan(s64[1, 3:]).all() and np.isnan(s32[1, 3:]).all()
    g64, g32 = dr.gain_from_s(s64), dr.gain_from_s(s32)
    rel = dr.gain_rel_bound(pred, tru, [5, 3], 0.01, taps, 1.0) - dr.exp2_rel_bound()       # the twin's exponential is exact
    ok = ~np.isnan(s64)
    err, bound = np.abs(g32 - g64)[ok], (rel * g64)[ok]
    assert not err[bound <= 0].any()                                      # a difference of exactly 0 carries no error
    ratio = (err[bound > 0] / bound[bound > 0]).max()
    print('gain twin nb=%d h=%d: worst error / bound %.3f' % (nb, h, ratio))
    assert ratio <= 1.0 and not g64[1, 3:].any() and not g32[1, 3:].any()
    assert (s64[ok] > -30).any() and (s64[ok] < 20).any()


def test_taps():
    import conversion
    for h in (0, 1, 8, 32):
        c = conversion.diff_smoothing_taps(h)
        assert c.dtype == np.float32 and c.shape == (2 * h + 1,) and np.array_equal(c, c[::-1]) and (c > 0).all()
        assert abs(float(c.astype(np.float64).sum()) - 1.0) <= (2 * h + 1) * 2.0 ** -25
        assert np.array_equal(c, dr.smoothing_taps(h))
        assert c.argmax() == h
    assert conversion.diff_smoothing_taps(0).tolist() == [1.0]
    pred, tru = _spectra(1, 3, 33, 4)
    s = dr.gain_s(pred, tru, None, 0.01, [1.0], 1.0, 1e9, 1e9)
    d = (np.maximum(pred, 0).astype(np.float64) - np.maximum(tru, 0)) / float(np.float32(0.01))
    assert np.array_equal(s, d)                                           # half_width 0: the difference itself
    for bad in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match='half_width'):
            conversion.diff_smoothing_taps(bad)


@pytest.mark.parametrize('nb,h', [(33, 8), (201, 32), (9, 8)])
def test_mirrored_edges_are_a_reflect_padded_convolution(nb, h):
    pred, tru = _spectra(1, 4, nb, nb)
    taps = dr.smoothing_taps(h)
    s = dr.gain_s(pred, tru, None, 0.01, taps, 1.0, 1e9, 1e9)[0]
    d = (np.maximum(pred[0], 0).astype(np.float64) - np.maximum(tru[0], 0)) / float(np.float32(0.01))
    dp = np.pad(d, ((0, 0), (h, h)), mode='reflect')                      # numpy's reflect: no edge repeat, h <= nb - 1
    want = np.stack([np.convolve(row, taps.astype(np.float64)[::-1], mode='valid') for row in dp])
    assert want.shape == s.shape and np.abs(s - want).max() <= 1e-12 * np.abs(want).max()
    assert dr.refl(np.array([-1, -2, nb, nb + 1, 2 * (nb - 1), -2 * (nb - 1) - 1]), nb).tolist() == [1, 2, nb - 2, nb - 3, 0, 1]


def test_clamps_and_alpha():
    pred = np.zeros((1, 2, 9), np.float32)
    tru = np.zeros((1, 2, 9), np.float32)
    pred[0, 0], tru[0, 1] = 0.9, 0.9                                      # +90 dB and -90 dB before the clamps
    pred[0, 1, 3] = -5.0                                                   # negative inputs count as 0
    for dtype in (np.float64, np.float32):
        s = dr.gain_s(pred, tru, None, 0.01, dr.smoothing_taps(1), 1.0, 20.0, 30.0, dtype=dtype)
        assert (s[0, 0] == 20).all() and (s[0, 1] == -30).all()
        g = dr.gain_from_s(s)
        assert np.abs(g[0, 0] - 10.0).max() <= 1e-5 and np.abs(g[0, 1] - 10.0 ** -1.5).max() <= 1e-7
        half = dr.gain_s(pred, tru, None, 0.01, dr.smoothing_taps(1), 0.5, 100.0, 100.0, dtype=dtype)
        assert np.abs(half[0, 0] - 45.0).max() <= 1e-4 and np.abs(half[0, 1] + 45.0).max() <= 1e-4
        g0 = dr.gain(*_spectra(1, 3, 9, 1), None, 0.01, dr.smoothing_taps(8), alpha=0.0, dtype=dtype)
        assert (g0 == 1.0).all()                                           # alpha 0: exactly 1 in every bin


# ------------------------------------------------------------------------------------------ the method's own check
LSD_WRITTEN = 3.70          # dB: what the float64 restatement gave when this test was written (of 16.14 dB source to target)


def test_two_vowels_move_to_the_target_and_keep_their_pitch():
    """The same pulse train (F0 gliding from 70 to 150 Hz over one second) through the formants of /a/ (source) and /i/
    (target); the gain from the restated front-end's two spectra at the defaults (half-width 8, alpha 1, +20 / -30 dB); the
    float64 filter.  The smoothed log-spectral distance (below 4 kHz, mean removed) of the output to the target must be at
    most a third of the source's and at most twice the value measured when this was written: 3.70 dB of 16.14 dB (the
    +20 dB clamp holds back the second formant of /i/, which sits in a valley of /a/).  The output's F0 by YIN
    (tests/f0_ref.py) stays within 20 cents of the source's on every voiced frame: measured 6.7 cents."""
    src, tgt, _ = dr.two_vowels(1.0)
    taps = dr.smoothing_taps(8)
    P_s, P_t = (dr.frontend_power_db(v, W, HOP).astype(np.float32)[None] for v in (src, tgt))
    G = dr.gain(P_t, P_s, None, 0.01, taps)[0]
    y = dr.stft_filter(src, G, W, HOP)
    L = len(y)
    d_src, d_out = dr.log_spectral_distance(src[:L], tgt[:L], W, HOP, taps), dr.log_spectral_distance(y, tgt[:L], W, HOP, taps)
    f_s, _ = f0_ref.yin(src[:L].astype(np.float32))
    f_y, _ = f0_ref.yin(y.astype(np.float32))
    voiced = f0_ref.fully_voiced_frames(np.ones(L, bool), HOP, 512, 267) & (f_s > 0)
    assert voiced.sum() >= 150 and (f_y[voiced] > 0).all()
    c = float(np.abs(f0_ref.cents(f_y[voiced], f_s[voiced])).max())
    print('two vowels: source to target %.3f dB, output to target %.3f dB; F0 within %.2f cents over %d frames'
          % (d_src, d_out, c, int(voiced.sum())))
    assert d_out <= d_src / 3.0 and d_out <= 2.0 * LSD_WRITTEN
    assert c <= 20.0


# ------------------------------------------------------------------------------------------ convert_diff_batch, host side
class _NoDecoder:
    encoder = object()


def test_convert_diff_batch_checks_before_any_gpu_call(monkeypatch):
    """Every refusal is a ValueError raised on the host; a valid call gets as far as the device check (made to fail here, so
    the test is the same with and without a GPU) -- nothing before it touched the GPU."""
    import torch
    import _vc
    import conversion
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    wav = np.zeros((3, 80000), np.float32)
    ok = dict(cfg_d=CFG, lens=[80000, 40000, 60000])
    st = (10, 5.0, 0.2)
    bad = [(dict(alpha=1.5), 'alpha'), (dict(alpha=-0.1), 'alpha'), (dict(alpha=float('nan')), 'alpha'), (dict(max_boost_db=-1.0), 'max_boost_db'),
           (dict(max_cut_db=-0.5), 'max_cut_db'), (dict(max_cut_db=float('inf')), 'max_cut_db'), (dict(half_width=33), 'half_width'),
           (dict(half_width=-1), 'half_width'), (dict(half_width=2.0), 'half_width'), (dict(pitch='target'), 'pitch'),
           (dict(pitch=2.5), 'pitch'), (dict(pitch='source'), 'stats'), (dict(pitch='source', stats_src=st), 'stats'),
           (dict(pitch=1.1, stats_src=st, stats_tgt=st), 'stats'), (dict(stats_src=st, stats_tgt=st), 'stats'),
           (dict(pitch=np.ones((3, 1199), np.float32)), 'contour'), (dict(pitch=np.ones((2, 1200), np.float32)), 'contour'),
           (dict(pitch=1.0, w_floor=0.0), 'w_floor'), (dict(pitch=1.0, f0_args=dict(hop_length=40)), 'f0_args'),
           (dict(utt_ids=[0, 1]), 'utt_ids'), (dict(window_batch=0), 'window_batch')]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            conversion.convert_diff_batch(_NoDecoder(), wav, **ok, **kw)
    with pytest.raises(ValueError, match='lens'):
        conversion.convert_diff_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[80000, 90000, 100])
    with pytest.raises(ValueError, match='wav'):
        conversion.convert_diff_batch(_NoDecoder(), wav[0], **ok)
    with pytest.raises(ValueError, match='cfg_d'):
        conversion.convert_diff_batch(_NoDecoder(), wav)
    with pytest.raises(ValueError, match='frames-1'):
        conversion.convert_diff_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[80000, 230, 60000])      # 3 frames: 160 samples <= 200
    for kw in (dict(), dict(pitch=1.2), dict(pitch='source', stats_src=st, stats_tgt=st), dict(pitch=np.ones((3, 1200), np.float32)),
               dict(out_sr=22050, wav_sr=8000, lens=[40000, 20000, 30000])):
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            conversion.convert_diff_batch(_NoDecoder(), wav, **dict(ok, **kw))
    for fn, args in ((conversion.diff_gain_batch, (np.zeros((2, 5, 201), np.float32), np.zeros((2, 5, 201), np.float32), [5, 4], 0.01)),):
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            fn(*args)
        for kw, msg in ((dict(alpha=2.0), 'alpha'), (dict(taps=[0.5, 0.5]), 'taps'), (dict(taps=np.ones(67) / 67), 'taps'),
                        (dict(max_boost_db=-1), 'max_boost_db')):
            with pytest.raises(ValueError, match=msg):
                fn(*args, **kw)
        with pytest.raises(ValueError, match='n_frames'):
            fn(args[0], args[1], [5, 6], 0.01)
        with pytest.raises(ValueError, match='shape'):
            fn(args[0], args[1][:, :4], [5, 4], 0.01)
    import audio_lib
    with pytest.raises(ValueError, match='gain'):
        audio_lib.stft_filter_batch(wav, [80000] * 3, np.ones((3, 10, 200), np.float32))
    with pytest.raises(ValueError, match='lens'):
        audio_lib.stft_filter_batch(wav, [80001, 5, 5], np.ones((3, 10, 201), np.float32))
    with pytest.raises(ValueError, match='n_frames'):
        audio_lib.stft_filter_batch(wav, [80000] * 3, np.ones((3, 10, 201), np.float32), n_frames=[11, 1, 1])
    with pytest.raises(_vc.VCError, match='needs a GPU'):
        audio_lib.stft_filter_batch(wav, [80000] * 3, np.ones((3, 10, 201), np.float32))


@pytest.mark.parametrize('t_e', [60, 3])
def test_n_use_and_n_samples_follow_convert_plan(t_e):
    """n_use = min(n_out, n_clip): whole converted windows, cut where the source ends (an utterance of 1001 frames is padded
    to 1200 and converted as three windows; the source covers 1001 of them) or where t_e cuts it."""
    import conversion
    lens = [int(s * 16000) for s in (3.2, 1.5, 5.0)]
    plan = conversion.convert_plan(lens, CFG, 0, t_e, True)
    n_use, n_samples = conversion.diff_frames(plan, 80)
    for b, L in enumerate(lens):
        n_src = 1 + L // 80
        assert n_use[b] == min(int(plan.N[b]) * 400, n_src, int(plan.n_e[b])) and n_use[b] <= n_src
        assert n_samples[b] == 80 * (n_use[b] - 1) <= L
    if t_e == 60:
        assert n_use.tolist() == [641, 301, 1001] and plan.n_out.tolist() == [800, 400, 1200]
    else:
        assert n_use.tolist() == [400, 301, 400]


def test_new_exports_are_declared_and_bound():
    import _vc
    lib = _vc.lib()
    for name in ('vc_spectral_diff_gain_f32', 'vc_stft_filter_workspace_bytes', 'vc_stft_filter_f32'):
        assert name in _vc._SIGS and hasattr(lib, name)
    assert lib.vc_stft_filter_workspace_bytes(None, 2, 5) == 0
    assert lib.vc_spectral_diff_gain_f32(None, None, None, 1, 1, 201, 0.01, 1.0, 20.0, 30.0, None, 17, None, None) == 1
    assert b'vc_spectral_diff_gain_f32' in lib.vc_last_error()
    assert lib.vc_stft_filter_f32(None, None, 10, None, None, None, 1, 1, None, 0, None, 0, None) == 1
    assert b'vc_stft_filter_f32' in lib.vc_last_error()
