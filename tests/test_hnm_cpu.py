"""The harmonic-plus-noise vocoder's numpy restatement (tests/hnm_ref.py) tested on its own, and the host-side argument checks
of its Python entry points: no GPU needed."""
import numpy as np
import pytest

import hnm_ref as R

SR, N, HOP = 16000, 400, 80
# the round trip measured on the float64 reference (test_round_trip_regression): rms dB at 120 Hz and at 200 Hz
ROUND_TRIP_RMS = {120.0: 0.851, 200.0: 1.914}
ROUND_TRIP_F = 26


def test_closed_form_phase_equals_accumulation():
    rng = np.random.default_rng(3)
    for b, hop in enumerate((1, 80, 256)):
        F = 40
        f0 = rng.uniform(60.0, 3900.0, F).astype(np.float32)
        f0[rng.random(F) < 0.3] = 0.0
        pl = R.plan(f0, F, SR, hop)
        ph = 0
        for f in range(F - 1):
            got = R.sample_phase(pl, hop, f, np.arange(hop))
            for j in range(hop):
                assert int(got[j]) == ph, (b, f, j)
                ph = (ph + int(pl['inc'][f]) + int(pl['slope'][f]) * j) % (1 << 32)
            assert ph == int(pl['phase'][f + 1])


def test_plan_fills_unvoiced_frames_and_flags():
    f0 = np.array([0, 0, 100, 0, 200, 0, 0], np.float32)
    pl = R.plan(f0, 6, SR, HOP)
    k = np.float32(2.0 ** 32 / SR)
    i100, i200 = int(np.rint(np.float32(100) * k)), int(np.rint(np.float32(200) * k))
    assert pl['inc'].tolist() == [i100, i100, i100, i100, i200, i200, 0]
    assert pl['voiced'].tolist() == [0, 0, 1, 0, 1, 0, 0] and pl['flags'] == 0
    assert pl['slope'][3] == (i200 - i100) // HOP and pl['slope'][5] == 0 and pl['phase'][6] == 0
    for bad in (39.0, 4001.0, np.nan, -100.0, np.inf):
        pl = R.plan(np.array([100, bad], np.float32), 2, SR, HOP)
        assert pl['flags'] == 1 and pl['voiced'].tolist() == [1, 0]
    pl = R.plan(np.array([40.0, 4000.0], np.float32), 2, SR, HOP)
    assert pl['flags'] == 0 and pl['voiced'].tolist() == [1, 1]
    pl = R.plan(np.zeros(5, np.float32), 5, SR, HOP)
    assert not pl['inc'].any() and not pl['phase'].any() and pl['flags'] == 0


def test_calibration_single_harmonic_at_a_bin_centre():
    """scale = 2 / sum(w): a stationary harmonic at a bin centre reads back from the STFT at the envelope's own value."""
    n_fft, hop, F, m = 256, 64, 12, 10
    w = R.window(n_fft, n_fft)
    f0 = np.full(F, SR * m / n_fft, np.float32)                    # 625 Hz: inc = m 2^24 exactly
    pl = R.plan(f0, F, SR, hop)
    assert int(pl['inc'][0]) == m << 24
    env = 0.37
    el = np.full((F, n_fft // 2 + 1), np.log(env))
    y = R.synth(el, np.zeros_like(el), pl, F, n_fft, hop, int(pl['inc'][0]) + 1, 2.0 / w.sum())[0]
    S = R.stft_mag(y, w, hop)[3:-3]
    el32 = np.float64(np.float32(np.log(env)))
    assert np.abs(S[:, m] / np.exp(el32) - 1.0).max() < 1e-9
    # ... and nowhere else, down to the float32 rounding of the window's values (the exact Hann window has zeros there)
    assert np.abs(np.delete(S, [m - 1, m, m + 1], axis=1)).max() < 1e-7


def test_envelope_identities():
    rng = np.random.default_rng(5)
    for n_fft in (16, 400):
        nb = n_fft // 2 + 1
        c = np.full((2, nb), 0.25, np.float32)
        E, th, bE, bth, _ = R.envelope(c, n_fft, 3, 4, 1e-5)
        assert np.abs(E - np.log(0.25)).max() < 1e-12 and np.abs(th).max() < 1e-12
        # order N/2 - 1 leaves out one cepstral coefficient, c_{N/2}: without it in the data, iters = 0 returns the data
        a = rng.normal(0.0, 1.0, (3, nb))
        w = np.full(nb, 2.0)
        w[0] = w[-1] = 1.0
        alt = (-1.0) ** np.arange(nb)
        a -= ((a * w * alt).sum(axis=1) / n_fft)[:, None] * alt[None, :]
        amp = np.exp(a).astype(np.float32)
        E = R.envelope(amp, n_fft, n_fft // 2 - 1, 0, 1e-5)[0]
        assert np.abs(E - np.log(amp.astype(np.float64))).max() < 1e-6
        # the true-envelope iteration never lowers the smoothed curve, and the floor is applied
        amp = np.exp(rng.normal(0.0, 1.5, (3, nb))).astype(np.float32)
        E0 = R.envelope(amp, n_fft, 3, 0, 1e-5)[0]
        E9 = R.envelope(amp, n_fft, 3, 9, 1e-5)[0]
        assert E9.mean() > E0.mean()
        assert np.array_equal(R.envelope(np.zeros((1, nb), np.float32), n_fft, 3, 2, 1e-3)[0],
                              R.envelope(np.full((1, nb), 1e-3, np.float32), n_fft, 3, 2, 1e-3)[0])
    # minimum phase of a one-pole system 1 / (1 - r z^-1)
    n_fft, r = 64, 0.5
    wk = 2.0 * np.pi * np.arange(n_fft // 2 + 1) / n_fft
    H = 1.0 / (1.0 - r * np.exp(-1j * wk))
    E, th = R.envelope(np.abs(H).astype(np.float32)[None], n_fft, n_fft // 2 - 1, 0, 1e-5)[:2]
    assert np.abs(th[0] - np.angle(H)).max() < 1e-6


def test_cosine_polynomial_error():
    z = np.linspace(-0.5, 0.5, 400001)
    assert np.abs(R.cos_turns_f64(z) - np.cos(2.0 * np.pi * z)).max() < R.COS_POLY_ERR
    assert np.abs(R.cos_turns_f64(z + 3.0) - np.cos(2.0 * np.pi * z)).max() < R.COS_POLY_ERR + 1e-12


def test_noise_reference_statistics():
    x = R.noise(7, 3, 1 << 16).astype(np.float64)
    assert np.array_equal(R.noise(7, 3, 100), R.noise(7, 3, 1 << 16)[:100])
    assert not np.array_equal(R.noise(7, 4, 100), R.noise(7, 3, 100))
    # mean of 2^16 unit-variance samples: sigma 2^-8; variance: sigma sqrt(0.8 / 2^16)
    assert abs(x.mean()) < 4 * 2.0 ** -8 and abs(x.var() - 1.0) < 4 * np.sqrt(0.8 / 65536)
    assert np.abs(x).max() <= np.sqrt(3.0)


@pytest.mark.parametrize('f0_hz', sorted(ROUND_TRIP_RMS))
def test_round_trip_regression(f0_hz):
    """The vowel (four-formant all-pole envelope, +-10 % vibrato) through envelope -> plan -> synthesis -> STFT -> envelope
    comes back to the envelope over the bins between 1.2 f0 and 7.4 kHz.  Measured on this reference: 0.851 dB rms (mean
    -0.305) at 120 Hz, 1.914 dB rms (mean -1.195) at 200 Hz, where the 25 ms window smears the vibrato of the upper
    harmonics.  The 1.5x margin covers the choice of vibrato phase, not rounding."""
    amp, f0, env = R.vowel(f0_hz, ROUND_TRIP_F)
    y = R.chain(amp, f0)[0]
    rms, mean = R.round_trip_db(y, env, f0_hz)
    print('round trip at %g Hz: rms %.3f dB, mean %.3f dB' % (f0_hz, rms, mean))
    assert abs(rms - ROUND_TRIP_RMS[f0_hz]) < 0.01
    amp, f0, env = R.vowel(f0_hz, ROUND_TRIP_F, phase0=1.0)
    assert R.round_trip_db(R.chain(amp, f0)[0], env, f0_hz)[0] < 1.5 * ROUND_TRIP_RMS[f0_hz]


def test_argument_errors_before_any_launch():
    import audio_lib
    amp = np.ones((2, 5, 201), np.float32)
    f0 = np.full((2, 5), 100.0, np.float32)
    bad = [dict(order=0), dict(order=200), dict(iters=-1), dict(floor=0.0), dict(floor=float('nan')), dict(n_fft=401),
           dict(n_frames=[5, 6]), dict(n_frames=[5])]
    for kw in bad:
        with pytest.raises(ValueError, match=' - ERROR, envelope_batch'):
            audio_lib.envelope_batch(amp, **kw)
    with pytest.raises(ValueError, match=' - ERROR, envelope_batch'):
        audio_lib.envelope_batch(amp[:, :, :200])
    for kw in (dict(f0_lo=0.0), dict(f0_hi=9000.0), dict(f0_lo=500.0, f0_hi=400.0), dict(hop_length=0), dict(hop_length=5000)):
        args = dict(n_frames=None, sr=SR, hop_length=HOP)
        args.update(kw)
        with pytest.raises(ValueError, match=' - ERROR, hnm_plan_batch'):
            audio_lib.hnm_plan_batch(f0, **args)
    with pytest.raises(ValueError, match=' - ERROR, noise_batch'):
        audio_lib.noise_batch([5, 11], 10)
    with pytest.raises(ValueError, match=' - ERROR, seed'):
        audio_lib.noise_batch([5, 10], 10, seed=-1)
    for kw in (dict(voiced_cutoff_hz=0.0), dict(voiced_cutoff_hz=8000.0, f0_lo=20.0), dict(noise_level=-1.0), dict(order=200),
               dict(utt_ids=[1]), dict(n_frames=[6, 5]), dict(seed=2 ** 64)):
        with pytest.raises(ValueError, match=' - ERROR'):
            audio_lib.hnm_synth_batch(amp, f0, **kw)
    with pytest.raises(ValueError, match=' - ERROR, hnm_synth_batch: f0'):
        audio_lib.hnm_synth_batch(amp, f0[:, :4])
    assert audio_lib.hnm_cutoff(4000.0, SR, N, 40.0) == (1 << 30, 100)
    assert audio_lib.hnm_cutoff(9000.0, SR, N, 40.0) == (1 << 31, 200)


def test_convert_hnm_batch_argument_errors_before_any_launch():
    import conversion
    wav = np.zeros((1, 16000), np.float32)
    cfg = dict(sample_rate=SR, hop_length=HOP)
    bad = [dict(cfg_d=None), dict(pitch=None), dict(pitch='target'), dict(pitch=3.0), dict(stats_src=(1, 5.0, 0.2)),
           dict(pitch=np.zeros((1, 10), np.float32), stats_src=(1, 5.0, 0.2), stats_tgt=(1, 5.2, 0.2)),
           dict(f0_args=dict(window=3)), dict(seed=-1)]
    for kw in bad:
        args = dict(cfg_d=cfg)
        args.update(kw)
        with pytest.raises(ValueError, match=' - ERROR'):
            conversion.convert_hnm_batch(None, wav, [16000], **args)
