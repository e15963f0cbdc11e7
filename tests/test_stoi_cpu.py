"""Intelligibility scoring without a GPU: the arithmetic of include/vc_hip.h ("Intelligibility") as tests/stoi_ref.py
restates it -- band table, framing, the fused three-frame gather, the scores' invariants, their behaviour on a noisy vowel,
SI-SDR against a constructed SNR -- the conditioning of every GPU case's kept list, and the host validation of
evaluation.stoi_batch / si_sdr_batch / stoi_bands."""
import numpy as np
import pytest

import stoi_cases as sc
import stoi_ref as sr

LOWER_EDGES = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]


def test_band_table_is_the_published_one():
    import evaluation
    tab = sr.bands()
    assert tab[:, 0].tolist() == LOWER_EDGES and int(tab[-1, 1]) == 219
    assert tab[:-1, 1].tolist() == tab[1:, 0].tolist()              # the bands tile [7, 219)
    pub = evaluation.stoi_bands()
    assert pub.dtype == np.int32 and pub.shape == (15, 2) and np.array_equal(pub, tab)
    assert np.array_equal(evaluation.stoi_bands(16000, 1024, 20, 100.0), sr.bands(16000, 1024, 20, 100.0))


def test_frame_counts_are_matlabs():
    import evaluation
    for L, F in ((0, 0), (255, 0), (256, 0), (257, 1), (384, 1), (385, 2), (512, 2), (513, 3)):
        assert sr.n_frames(L) == F == evaluation.stoi_frames(L) == len(range(0, max(L - sr.W, 0), sr.H)), L
    for K in (1, 2, 31):
        assert sr.n_frames(sc.len_for_frames(K)) == K and sr.n_frames(sc.len_for_frames(K) - 1) == K - 1


def test_window_is_hanning_without_its_zero_endpoints():
    w = sr.window()
    n = np.arange(sr.W)
    assert len(w) == sr.W and w.min() > 0 and np.allclose(w, w[::-1], atol=1e-15)
    assert np.abs(w - (0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 1) / (sr.W + 1)))).max() < 1e-15


@pytest.mark.parametrize('name', sc.BAND_CASES)
def test_fused_gather_is_the_materialised_signal(name):
    """M = K - 1, and frame m of the silence-removed signal is the gather through idx[m - 1], idx[m], idx[m + 1]: the
    identity vc_stoi_bands_f32 relies on, to 1e-12 relative in float64."""
    x, _ = sc.band_case(name)
    idx = sr.kept(sr.energies(x))
    a, b = sr.frames_materialised(x, idx), sr.frames_fused(x, idx)
    assert a.shape == b.shape == (max(len(idx) - 1, 0), sr.W)
    assert len(sr.silence_removed(x, idx)) == ((len(idx) + 1) * sr.H if len(idx) else 0)
    if name.startswith('K'):
        assert len(idx) == int(name[1:])
    if name == 'gaps':
        assert (np.diff(idx) > 1).any(), 'the case must cross non-adjacent frames'
    if len(a):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_stockham_twin_is_the_transform():
    z = np.random.RandomState(1).standard_normal((5, sr.W))
    want = np.fft.fft(z, sr.NFFT, axis=1)
    re, im = sr.stockham(z, np.float64)
    assert np.abs(re + 1j * im - want).max() < 1e-12
    re, im = sr.stockham(z, np.float32)
    assert np.abs(re + 1j * im - want).max() < 1e-4


def test_impulse_and_cosine_in_closed_form():
    """An impulse inside two kept frames: every bin of frame 0 has the magnitude (w[168] + w[40]) w[168] A, so
    T[0, j] = that times sqrt(hi - lo).  A bin-centred cosine: the direct sum over the analytic frame."""
    tab, w = sr.bands(), sr.window()
    x, p, A = sc.impulse()
    idx = sr.kept(sr.energies(x))
    assert idx.tolist() == [4, 5]
    T = sr.band_T(x, idx)
    want = (w[168] + w[40]) * w[168] * A * np.sqrt(tab[:, 1] - tab[:, 0])
    assert T.shape == (1, 15) and np.abs(T[0] - want).max() <= 1e-12 * want.max()
    x = sc.cosine()
    idx = sr.kept(sr.energies(x))
    assert idx.tolist() == [0, 1, 2, 3]
    T = sr.band_T(x, idx)
    n = np.arange(sr.W)
    for m in range(3):
        g = w * np.where(n < sr.H, (w[(n + sr.H) % sr.W] if m else 0.0) + w, w + w[(n - sr.H) % sr.W])
        z = g * x[m * sr.H:m * sr.H + sr.W]                         # every frame is kept: x_sil's frame m lies at m H
        X = np.array([np.sum(z * np.exp(-2j * np.pi * k * n / sr.NFFT)) for k in range(257)])
        want = np.sqrt([np.sum(np.abs(X[lo:hi]) ** 2) for lo, hi in tab])
        assert np.abs(T[m] - want).max() <= 1e-12 * want.max()
    assert int(np.argmax(T[1])) == int(np.nonzero((tab[:, 0] <= 40) & (40 < tab[:, 1]))[0][0])


@pytest.mark.parametrize('extended', (False, True))
def test_identity_and_scale_invariance(extended):
    x, y = sc.vowel_pair(5)
    assert abs(sr.stoi(x, x, extended=extended) - 1.0) <= 1e-12
    base = sr.stoi(x, y, extended=extended)
    for e in (-10, 10):
        assert abs(sr.stoi(x, y * 2.0 ** e, extended=extended) - base) <= 1e-12, e


def test_scores_fall_with_the_snr_on_a_noisy_vowel():
    """A modulated three-formant vowel in white noise at 20 / 10 / 0 / -10 dB: STOI and ESTOI fall strictly; SI-SDR is the
    SNR to the fraction of a dB that the noise's chance correlation with the vowel leaves."""
    rows = []
    for snr in (20, 10, 0, -10):
        x, y = sc.vowel_pair(snr)
        s, seg, idx, _, _ = sr.stoi(x, y, detail=True)
        e = sr.stoi(x, y, extended=True)
        d = sr.si_sdr(x, y)[0]
        rows.append((s, e))
        print('MEASURED vowel at %+d dB: STOI %.3f ESTOI %.3f SI-SDR %.2f dB over %d segments of %d kept frames'
              % (snr, s, e, d, len(seg), len(idx)))
        assert abs(d - snr) < 1.0 and len(seg) == len(idx) - sr.N_SEG
    for a, b in zip(rows[:-1], rows[1:]):
        assert a[0] > b[0] and a[1] > b[1]
    assert all(-1.0 <= v <= 1.0 for r in rows for v in r)


def test_no_segment_gives_zero_not_nan():
    x = sc.noise(sc.len_for_frames(30), 1)                          # K = 30, M = 29, S = 0
    s, seg, idx, Tx, _ = sr.stoi(x, x, detail=True)
    assert len(idx) == 30 and Tx.shape == (29, 15) and len(seg) == 0 and s == 0.0
    assert sr.stoi(np.zeros(5000), np.zeros(5000)) == 0.0 and sr.stoi(np.zeros(10), np.zeros(10)) == 0.0


@pytest.mark.parametrize('zero_mean', (True, False))
def test_si_sdr_is_the_constructions_snr(zero_mean):
    rng = np.random.RandomState(5)
    x = rng.standard_normal(4000)
    if zero_mean:
        x -= x.mean()
    for snr in (-5.0, 0.0, 17.5, 40.0):
        n = rng.standard_normal(4000)
        if zero_mean:
            n -= n.mean()
        n -= x * np.dot(n, x) / np.dot(x, x)                        # n orthogonal to x
        n *= np.sqrt(np.dot(x, x) / np.dot(n, n) / 10.0 ** (snr / 10.0))
        got, valid = sr.si_sdr(x, 0.37 * (x + n), zero_mean=zero_mean)
        assert valid == 1 and abs(got - snr) <= 1e-9, (snr, got)
    assert sr.si_sdr(np.zeros(9), np.ones(9), zero_mean=False) == (0.0, 0)
    assert sr.si_sdr(x, x, zero_mean=zero_mean) == (np.inf, 1) and sr.si_sdr(x, 0.0 * x)[0] == -np.inf and sr.si_sdr(x, x, 0) == (0.0, 0)


def test_float32_twins_stay_near_float64():
    x, y = sc.band_case('K31')
    idx = sr.kept(sr.energies(x))
    T64, T32, bound = sr.band_T(x, idx), sr.band_T(x, idx, dtype=np.float32), sr.band_bound(x, idx)
    r = float((np.abs(T32 - T64) / bound).max())
    print('MEASURED band twin against float64: worst error / bound %.3f' % r)
    assert r <= 1.0


def test_every_gpu_case_has_a_well_conditioned_kept_list():
    """No frame energy within a relative 1e-3 of its keep threshold: float32 rounding of the energies (a few 1e-7) cannot
    move a frame across it, so the device's kept list is required to be exact."""
    worst = np.inf
    for name, x, L in sc.every_reference():
        m = sr.threshold_margin(sr.energies(x, L))
        worst = min(worst, m)
        assert m > 1e-3, (name, m)
    print('MEASURED nearest frame energy to its threshold: relative distance %.3g' % worst)


# ------------------------------------------------------------------------------------------ host validation (no GPU)
def _pair(B=2, L=600):
    x = np.zeros((B, L), np.float32)
    return x, x.copy()


@pytest.mark.parametrize('kw', (dict(deg=np.zeros((2, 599), np.float32)), dict(ref=np.zeros(600, np.float32)), dict(lens=[600]),
                                dict(lens=[600, 601]), dict(lens=[-1, 5]), dict(lens=[1.5, 2.0]), dict(wav_sr=0), dict(wav_sr=16000.0),
                                dict(dyn_range=0), dict(dyn_range=float('nan')), dict(dyn_range='40'), dict(dyn_range=1e-9),
                                dict(wav_sr=16000, res_type='nope'), dict(wav_sr=16000, lens=[0, 600]),
                                dict(ref=np.zeros((1, 128 * 16400 + 300), np.float32), deg=np.zeros((1, 128 * 16400 + 300), np.float32))))
def test_stoi_batch_refuses_on_the_host(kw):
    import evaluation
    ref, deg = _pair()
    args = dict(ref=ref, deg=deg)
    args.update(kw)
    with pytest.raises(ValueError):
        evaluation.stoi_batch(**args)


@pytest.mark.parametrize('kw', (dict(deg=np.zeros((3, 600), np.float32)), dict(ref=np.zeros((2, 0), np.float32)), dict(lens=[1, 2, 3]),
                                dict(lens=[700, 1]), dict(zero_mean=1), dict(zero_mean=None)))
def test_si_sdr_batch_refuses_on_the_host(kw):
    import evaluation
    ref, deg = _pair()
    args = dict(ref=ref, deg=deg)
    args.update(kw)
    with pytest.raises(ValueError):
        evaluation.si_sdr_batch(**args)


@pytest.mark.parametrize('kw', (dict(fs=0), dict(n_fft=511), dict(n_bands=0), dict(n_bands=1.5), dict(f_min=0.0), dict(f_min='a')))
def test_stoi_bands_refuses(kw):
    import evaluation
    with pytest.raises(ValueError):
        evaluation.stoi_bands(**kw)


def test_valid_calls_need_a_gpu():
    """Past the host checks both calls reach the device: without one they raise VCError like their neighbours."""
    import torch
    import _vc
    import evaluation
    if torch.cuda.is_available():
        return                                                      # tests/test_stoi_gpu.py runs the calls
    ref, deg = _pair()
    with pytest.raises(_vc.VCError):
        evaluation.stoi_batch(ref, deg, [600, 300])
    with pytest.raises(_vc.VCError):
        evaluation.si_sdr_batch(ref, deg)
