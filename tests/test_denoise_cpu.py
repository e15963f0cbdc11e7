"""Noise suppression without a GPU: the numpy restatement of tests/denoise_ref.py held to what the device tests need of it
(the E1 form, the three exactness properties of the float32 twin, the share of lanes near the 0.99 guard), its behaviour on a
noisy synthetic vowel, and the host checks of every new Python call."""
import functools

import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref as dr
import vocoder_kernels_ref as vr
from test_convert_batch_cpu import CFG
from test_convert_errors_cpu import LENS, WAV, _NoDecoder

HOP, SR, LEAD, FLOOR_DB = 80, 16000, 0.6, 20.0
W = vr.device_window(vr.padded_window(400, 400))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ E1
def test_e1_form_against_scipy():
    """Abramowitz & Stegun give |error| < 2e-7 for 5.1.53 (absolute, so 9.2e-7 of E1(1) = 0.2194) and 5.1.56 is tighter; the
    float32 evaluation adds the roundings of a six-term Horner chain, a logarithm, an exponential and two divisions, taken as
    16 u.  Measured here: 1.9e-7 in float64, 4.6e-7 in float32."""
    from scipy.special import exp1
    x = np.exp(np.linspace(np.log(1e-6), np.log(30.0), 20001))
    e64 = float(np.abs(dr.e1(x) / exp1(x) - 1.0).max())
    x32 = x.astype(np.float32)
    e32 = float(np.abs(dr.e1(x32, np.float32).astype(np.float64) / exp1(x32.astype(np.float64)) - 1.0).max())
    print('MEASURED E1 max relative error over [1e-6, 30]: float64 %.2e float32 %.2e' % (e64, e32))
    assert dr.e1(x32, np.float32).dtype == np.float32
    assert e64 <= 2e-7 / 0.2194 and e32 <= 2e-7 / 0.2194 + 16 * dr.U


# ------------------------------------------------------------------------------------------ exactness of the twin
def _exact_inputs():
    P, counts, noise0 = dc.inputs(65, 'long')
    return P, counts, noise0


@pytest.mark.parametrize('rule', (0, 1))
def test_twin_freezes_the_noise_bit_for_bit(rule):
    P, counts, noise0 = _exact_inputs()
    g, s = dr.noise_gain(P, counts, noise0, dr.config(rule=rule, a_noise=1.0), dtype=np.float32)
    for b, n in enumerate(np.clip(counts, 0, P.shape[1])):
        assert np.array_equal(_bits(s[b, :n]), _bits(np.broadcast_to(np.maximum(noise0[b], np.float32(dr.FLT_MIN)), (n, 65))))
        assert not s[b, n:].any() and not g[b, n:].any()


@pytest.mark.parametrize('m', (-20, 20))
@pytest.mark.parametrize('with_noise0', (False, True))
def test_twin_scales_exactly_by_powers_of_two(m, with_noise0):
    P, counts, noise0 = _exact_inputs()
    k = np.float32(2.0 ** m)
    n0 = noise0 if with_noise0 else None
    g, s = dr.noise_gain(P, counts, n0, dr.config(), dtype=np.float32)
    g2, s2 = dr.noise_gain(P * k, counts, None if n0 is None else n0 * k, dr.config(), dtype=np.float32)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(s * k), _bits(s2)) and s.max() > 0


def closed_form_gain(P, counts, noise0, cfg):
    """Rule 0 with a_dd == 0, a_noise == 1 and noise0 given, written out directly in float32: no recursion is left."""
    f = np.float32
    with np.errstate(all='ignore'):
        s = np.maximum(noise0, f(dr.FLT_MIN))[:, None, :]
        g = np.minimum(P / s, f(cfg['gamma_max']))
        xi = np.maximum(np.maximum(g - f(1.0), f(0.0)), f(cfg['xi_min']))
        G = np.minimum(np.maximum(xi / (f(1.0) + xi), f(cfg['gain_min'])), f(1.0))
    for b, n in enumerate(counts):
        G[b, min(max(n, 0), P.shape[1]):] = 0.0
    return G


def test_twin_without_transcendentals_is_the_closed_form():
    P, counts, noise0 = _exact_inputs()
    cfg = dr.config(rule=0, a_dd=0.0, a_noise=1.0)
    g, _ = dr.noise_gain(P, counts, noise0, cfg, dtype=np.float32)
    want = closed_form_gain(P, counts, noise0, cfg)
    assert g.dtype == np.float32 and np.array_equal(_bits(g), _bits(want))
    assert len(np.unique(g)) > 1000 and (g == np.float32(cfg['gain_min'])).any() and (g > 0.9).any()


def test_all_zero_power_stays_finite():
    for rule in (0, 1):
        for T in (np.float64, np.float32):
            g, s = dr.noise_gain(np.zeros((1, 12, 9)), None, None, dr.config(rule=rule), dtype=T)
            assert np.isfinite(g).all() and np.isfinite(s).all() and (g >= 0.1 * (1 - 1e-6)).all() and (s == dr.FLT_MIN).all()


@pytest.mark.parametrize('nb', dc.NBINS)
def test_general_cases_stay_clear_of_the_guard(nb):
    """At most 5 % of a case's lanes may be left out of the device comparison; the committed seed keeps every case there."""
    for rule in (0, 1):
        for kind in dc.LAUNCHES:
            for with_noise0 in (False, True):
                g64, s64, out, bg, bs = dc.reference(nb, rule, kind, with_noise0)
                share = dc.lanes_left_out(out, dc.LAUNCHES[kind][1])
                print('MEASURED twin nb=%d rule=%d %s noise0=%d: 4 x distance gain %.2e noise (relative) %.2e; lanes left out %.3f'
                      % (nb, rule, kind, with_noise0, bg, bs, share))
                assert share <= 0.05 and 0.0 < bg < 1e-3 and 0.0 < bs < 1e-3


# ------------------------------------------------------------------------------------------ behaviour
@functools.lru_cache(maxsize=None)
def vowel_case(hz, snr_db):
    """One noisy vowel through the float64 restatement at the defaults: its five figures."""
    clean, noise = dr.noisy_vowel(hz, snr_db, seed=int(hz) + snr_db, lead=LEAD)
    x = clean + noise
    P, F, _ = dr.power(x, len(x), None, 1 + len(x) // HOP, W, HOP)
    cfg = dr.config()
    g, s = dr.noise_gain(P[None], None, None, cfg)
    psd = dr.true_psd(noise, W)
    snr_in, snr_out = dr.snr_figures(clean, noise, g[0], W, HOP, int(LEAD * SR))
    att, expected, bias = dr.lead_figures(P, g[0], s[0], psd, int(LEAD * SR) // HOP, cfg)
    return snr_in, snr_out, dr.psd_error_db(s[0], F, psd), att, expected, bias


@pytest.mark.parametrize('snr_db', (0, 10, 20))
@pytest.mark.parametrize('hz', (120.0, 210.0))
def test_reference_behaviour_on_a_noisy_vowel(hz, snr_db):
    """A three-formant vowel with vibrato behind 0.6 s of noise alone, white noise at 0, 10 and 20 dB, defaults throughout.
    The output SNR exceeds the input SNR; the final noise estimate is within 3 dB of the true level; the noise-only lead is
    attenuated within 1 dB of floor_db minus the tracker's bias, where "minus the bias" is made exact by
    denoise_ref.lead_figures: the attenuation the same rule gives on the same frames with the noise level frozen at what the
    tracker believes it to be.  Measured at the defaults: SNR +3.6 to +9.4 dB, level error -0.2 to -1.1 dB, 16.2 to 16.8 dB of
    attenuation at the 20 dB floor (the rule alone leaves 2 dB: the periodogram's exponential tail passes above the floor;
    the tracker's 1 dB underestimate costs the rest)."""
    snr_in, snr_out, psd_err, att, expected, bias = vowel_case(hz, snr_db)
    print('MEASURED vowel %g Hz at %d dB: SNR %.2f -> %.2f dB; final noise level %+.2f dB; lead attenuation %.2f dB, expected %.2f dB '
          'at bias %+.2f dB (floor %g dB)' % (hz, snr_db, snr_in, snr_out, psd_err, att, expected, bias, FLOOR_DB))
    assert abs(snr_in - snr_db) < 0.5
    assert snr_out > snr_in
    assert abs(psd_err) <= 3.0
    assert abs(att - expected) <= 1.0 and expected <= FLOOR_DB + 1e-9


def test_power_restatement_is_the_vocoder_reference_stft():
    rng = np.random.RandomState(0)
    x = rng.standard_normal(1000)
    P, F, bound = dr.power(x, 1000, None, 20, W, HOP)
    assert F == 13 and np.allclose(P[:F], np.abs(vr.stft_wave(x, W, HOP)) ** 2, rtol=1e-12, atol=0) and not P[F:].any()
    assert (bound[:F] > 0).all() and (bound[:F] < 1e-3 * P[:F].max()).all()
    assert dr.frames_of(200, None, 20, 400, HOP) == 0 and dr.frames_of(1000, 3, 20, 400, HOP) == 0      # 160 samples <= 200
    assert dr.frames_of(1000, -2, 20, 400, HOP) == 0 and dr.frames_of(1000, 4, 20, 400, HOP) == 4
    assert dr.frames_of(1040, 99, 13, 400, HOP) == 13 and dr.frames_of(1040, None, 20, 400, HOP) == 14


# ------------------------------------------------------------------------------------------ host checks
def test_smoothing_carries_the_papers_constants_to_this_hop():
    import enhance
    a_spp, a_noise = enhance.smoothing(256, 16000)
    assert abs(a_spp - 0.9) < 1e-4 and abs(a_noise - 0.8) < 1e-4                  # the paper's 16 ms hop
    a_spp, a_noise = enhance.smoothing(80, 16000)
    assert abs(a_spp - 0.9 ** (5.0 / 16.0)) < 1e-4 and abs(a_noise - 0.8 ** (5.0 / 16.0)) < 1e-4
    assert (a_spp, a_noise) == dr.smoothing(80, 16000)
    for bad in (dict(hop_length=0), dict(sr=-1), dict(tau_spp_ms=0.0), dict(tau_noise_ms=float('nan')), dict(hop_length='80')):
        with pytest.raises(ValueError, match='smoothing'):
            enhance.smoothing(**dict(dict(hop_length=80, sr=16000), **bad))


def test_gain_cfg_is_the_references_configuration():
    import enhance
    c, r = enhance.gain_cfg('x'), dr.config()
    for k in ('rule', 'n_init'):
        assert getattr(c, k) == r[k]
    for k in ('a_spp', 'a_noise', 'a_dd', 'xi_h1', 'xi_min', 'gain_min', 'gamma_max'):
        assert getattr(c, k) == np.float32(r[k]), k
    assert enhance.gain_cfg('x', rule='wiener').rule == 0


BAD_GAIN = [dict(rule='mmse'), dict(rule=1), dict(n_init=0), dict(n_init=2.5), dict(a_spp=1.5), dict(a_spp=-0.1), dict(a_noise=0.0),
            dict(a_noise=1.01), dict(a_dd=2.0), dict(a_dd=float('nan')), dict(xi_h1_db=float('inf')), dict(xi_min_db='low'),
            dict(floor_db=-1.0), dict(gamma_max=0.0), dict(gamma_max=float('nan'))]


@pytest.mark.parametrize('bad', BAD_GAIN, ids=lambda d: '%s=%r' % next(iter(d.items())))
def test_gain_keywords_are_checked_on_the_host(bad):
    import enhance
    P = np.ones((2, 5, 9), np.float32)
    with pytest.raises(ValueError, match='noise_gain_batch'):
        enhance.noise_gain_batch(P, [5, 3], **bad)
    with pytest.raises(ValueError, match='denoise_batch'):
        enhance.denoise_batch(np.zeros((2, 800), np.float32), [800, 500], **bad)
    with pytest.raises(ValueError, match='convert_batch: denoise'):
        import conversion
        conversion.convert_batch(_NoDecoder(), WAV, LENS, CFG, denoise=bad)


def test_shapes_and_counts_are_checked_on_the_host():
    import torch
    import audio_lib
    import enhance
    import _vc
    x = np.zeros((2, 800), np.float32)
    P = np.ones((2, 5, 9), np.float32)
    for call, what in ((lambda **k: audio_lib.stft_power_batch(**k), 'stft_power_batch'), (lambda **k: enhance.denoise_batch(**k), 'denoise_batch')):
        for bad in (dict(wav=x[0]), dict(lens=[800]), dict(lens=[800, 801]), dict(lens=[800, -1]), dict(lens=[800.0, 5.0]),
                    dict(n_frames=[11, 12]), dict(n_frames=[3]), dict(hop_length=0), dict(win_length=0), dict(n_fft=200), dict(n_fft=401),
                    dict(n_fft=8192), dict(hop_length=500), dict(wav=np.zeros((65536, 1), np.float32), lens=None)):
            with pytest.raises(ValueError, match=what):
                call(**dict(dict(wav=x, lens=[800, 500]), **bad))
    with pytest.raises(ValueError, match='denoise_batch'):
        enhance.denoise_batch(np.zeros((2, 40), np.float32), [40, 40])            # under one hop: no output sample
    with pytest.raises(ValueError, match='unknown'):
        enhance.denoise_batch(x, [800, 500], floor=20)
    for bad in (dict(noise0=np.ones((2, 8), np.float32)), dict(noise0=np.ones(9, np.float32))):
        with pytest.raises(ValueError, match='noise0'):
            enhance.noise_gain_batch(P, [5, 3], **bad)
    with pytest.raises(ValueError, match='noise0'):
        enhance.denoise_batch(x, [800, 500], noise0=np.ones((2, 9), np.float32))  # 201 bins at the defaults
    for bad in (dict(power=P[0]), dict(power=np.ones((2, 5, 1), np.float32)), dict(power=np.ones((2, 5, 2050), np.float32)),
                dict(n_frames=[5]), dict(n_frames=[5, 6]), dict(n_frames=[5, -1])):
        with pytest.raises(ValueError, match='noise_gain_batch'):
            enhance.noise_gain_batch(**dict(dict(power=P, n_frames=[5, 3]), **bad))
    if not torch.cuda.is_available():                                              # a valid call ends at the missing GPU
        for call in (lambda: audio_lib.stft_power_batch(x, [800, 500]), lambda: enhance.noise_gain_batch(P, [5, 3]),
                     lambda: enhance.denoise_batch(x, [800, 500], rule='wiener', return_noise=True)):
            with pytest.raises(_vc.VCError, match='needs a GPU'):
                call()


ENTRIES = (('convert_batch', {}), ('convert_duration_batch', dict(rate=1.25)), ('convert_pitch_batch', dict(pitch=1.2)),
           ('convert_hnm_batch', {}), ('convert_diff_batch', {}), ('convert_diff_duration_batch', dict(rate=1.25)),
           ('convert_postfilter_batch', dict(model=object())))


@pytest.mark.parametrize('entry,kw', ENTRIES, ids=[e for e, _ in ENTRIES])
def test_denoise_argument_of_every_entry_point_is_settled_before_the_gpu(entry, kw):
    """A bad denoise= is a ValueError and a good one reaches the GPU check, with a decoder that may not be touched; the cut to
    whole hops happens on the host too: 239 samples pass the plain length check (> n_fft//2 = 200) and fall to 160 with
    denoise on."""
    import torch
    import conversion
    import _vc
    fn = getattr(conversion, entry)
    for bad in ('yes', 1, dict(floor=3), dict(return_noise=True), dict(noise0=np.ones((3, 7), np.float32)), dict(a_noise=0.0)):
        with pytest.raises(ValueError, match=entry + ': denoise'):
            fn(_NoDecoder(), WAV, LENS, CFG, denoise=bad, **kw)
    short = [LENS[0], LENS[1], 239]
    with pytest.raises(ValueError, match='whole hops'):
        fn(_NoDecoder(), WAV, short, CFG, denoise=True, **kw)
    if not torch.cuda.is_available():
        for good in (None, False, True, dict(rule='wiener', floor_db=12.0), dict(noise0=np.ones((3, 201), np.float32))):
            with pytest.raises(_vc.VCError, match='needs a GPU'):
                fn(_NoDecoder(), WAV, LENS, CFG, denoise=good, **kw)


def test_lengths_are_cut_to_whole_hops_only_with_denoise():
    import conversion
    args = ('t', _NoDecoder(), WAV, [80000, 40079, 60001], CFG, 0, 60, True, None, 64, True, None, None, None, 'kaiser_best')
    plain, cut = conversion._convert_host(*args), conversion._convert_host(*args, denoise=True)
    assert plain.h_lens.tolist() == [80000, 40079, 60001] and cut.h_lens.tolist() == [80000, 40000, 60000]
    assert plain.denoise is None and cut.denoise is not None and cut.denoise[1] is None
    assert np.array_equal(plain.plan.n_out, cut.plan.n_out) and np.array_equal(plain.plan.n_clip, cut.plan.n_clip)
    assert conversion._convert_host(*args, denoise=False).denoise is None
