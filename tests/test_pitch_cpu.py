"""Pitch conversion, host side (include/vc_hip.h, "Pitch"): the numpy restatement of
tests/pitch_ref.py against facts that do not go through it, and the host path of conversion.pitch_tables, f0_stats_batch
and f0_transform against numpy.  No GPU."""
import numpy as np
import pytest
import torch

import f0_ref
import f0_track_ref
import pitch_ref as pr

Q = pr.Q


def random_tables(rng, F, wild=0.1):
    """period_q, ratio_q [F]: periods of 16 to 1,024 samples, ratios of 0.5 to 2, some of either beyond the clamps."""
    per = (rng.uniform(16, 1024, F) * Q).astype(np.int64)
    rat = (2.0 ** rng.uniform(-1, 1, F) * Q).astype(np.int64)
    for t in (per, rat):
        k = rng.rand(F) < wild
        t[k] = rng.choice([0, -5, 1, 2 ** 31 - 1, -2 ** 31, 15 * Q, 1025 * Q, 3 * Q], int(k.sum()))
    return per.astype(np.int32), rat.astype(np.int32)


CASES = [(n, hop, F) for n in (1, 15, 16, 17, 79, 80, 81, 1023, 1025, 4097, 20000) for hop, F in ((80, 1 + n // 80), (1, 300), (255, 1), (80, 500))]


def test_the_frame_wise_closed_form_is_the_mark_recurrence():
    rng = np.random.RandomState(1)
    for n, hop, F in CASES:
        per, rat = random_tables(rng, F)
        for T in pr.clamp_tables(per, rat):
            assert pr.marks_by_frame(T, n, hop) == pr.marks(T, n, hop), (n, hop, F)


def test_marks_increase_by_at_least_16_samples_and_stay_below_the_bound():
    rng = np.random.RandomState(2)
    for n, hop, F in CASES:
        per, rat = random_tables(rng, F, wild=0.5)
        P, S = pr.clamp_tables(per, rat)
        assert min(P) >= 16 * Q and max(P) <= 1024 * Q and min(S) >= 16 * Q and max(S) <= 2048 * Q
        for T in (P, S):
            m = np.array(pr.marks(T, n, hop))
            assert m[0] == 0 and m[-1] < n and len(m) <= n // 16 + 1
            assert len(m) < 2 or np.diff(m).min() >= 16
        p = pr.plan(per, rat, n, hop)
        assert (p.h[:p.J] >= 16).all() and (p.h[:p.J] <= 1024).all() and (p.h[p.J:] == -1).all() and (p.a[p.K:] == -1).all()
        assert set(p.src[:p.J].tolist()) <= set(p.a[:p.K].tolist())


def test_the_nearest_mark_rule_and_its_tie():
    a = [0, 100, 200]
    assert [pr.nearest(a, v) for v in (0, 49, 50, 51, 150, 151, 200, 999)] == [0, 0, 0, 1, 1, 2, 2, 2]
    # analysis period 100, ratio 2: the synthesis marks 50, 150 lie half way and go to the LOWER analysis mark
    p = pr.plan(np.full(4, 100 * Q), np.full(4, 2 * Q), 400, 80)
    assert p.a[:p.K].tolist() == [0, 100, 200, 300] and p.s[:p.J].tolist() == [0, 50, 100, 150, 200, 250, 300, 350]
    assert p.src[:p.J].tolist() == [0, 0, 100, 100, 200, 200, 300, 300] and (p.h[:p.J] == 100).all()


def test_ratio_one_copies_the_analysis_marks():
    rng = np.random.RandomState(3)
    for n, hop, F in CASES:
        per, _ = random_tables(rng, F)
        p = pr.plan(per, np.full(F, Q), n, hop)
        assert p.K == p.J and np.array_equal(p.s, p.a) and np.array_equal(p.src, p.s)


@pytest.mark.parametrize('contour', ['constant', 'varying'])
def test_identity_tables_return_the_signal_up_to_the_last_mark(contour):
    """Ratio 1 in float64: y == x wherever D >= w_floor.  Those samples are stated here: all of [0, s_{J-1}] -- between two
    marks of one frame the two windows add up to about 1, and a mark itself has weight 1 -- while the tail after the last
    mark has one falling window only and is damped by definition."""
    rng = np.random.RandomState(4)
    n, hop = 6070, 80
    F = 1 + n // hop
    f0 = np.full(F, 131.0) if contour == 'constant' else 120.0 * 2.0 ** (0.3 * np.sin(np.arange(F) / 9.0))
    per, rat = pr.tables(f0, 16000, ratio=1.0)
    x = rng.standard_normal(n + 50)
    y, D, p = pr.shift(x, n, per, rat, hop, dtype=np.float64)
    last = int(p.s[p.J - 1])
    live = D[:n] >= 0.5
    assert live[:last + 1].all() and not live.all()
    G = pr.coverage(len(x), n, p)[:n][live].max()
    assert np.abs(y[:n][live] - x[:n][live]).max() <= (2 * G + 1) * 2.0 ** -53 * np.abs(x[:n][live]).max()
    assert not y[n:].any() and (np.abs(y[:n][~live]) <= np.abs(x[:n][~live])).all()


# The nine cases (90, 120, 210 Hz by 0.8, 1.25, 1.5) on the restatement alone, measured by the YIN tracker's numpy
# restatement (f0_ref.yin, float64): all nine lie within 1.5 cents.  The Viterbi tracker's restatement (f0_track_ref.track)
# agrees to the last digit in seven; in the two of OCTAVE_LOW it reports the octave BELOW (-1200.0 and -1199.8 cents)
# although the dip at the true period is the deeper one (d' 0.037 against 0.059, 0.067 against 0.109 at a frame in the
# middle): marks are whole samples, so the grain pattern (3 synthesis marks per 2 analysis marks, 5 per 4) repeats every few
# periods and leaves a dip at twice the period that its path takes.  All nine are asserted for YIN, the seven others for
# the Viterbi tracker as well; the two are printed.
VOWEL_CASES = [(hz, r) for hz in (90.0, 120.0, 210.0) for r in (0.8, 1.25, 1.5)]
OCTAVE_LOW = {(90.0, 1.5), (120.0, 1.25)}
_tracked = {}


def tracked_vowel(hz, n=8000):
    if hz not in _tracked:
        x = pr.vowel(np.full(n, hz)).astype(np.float32)
        _tracked[hz] = (x, f0_track_ref.track(x)[0])
    return _tracked[hz]


@pytest.mark.parametrize('hz,ratio', VOWEL_CASES)
def test_a_vowels_fundamental_moves_by_the_ratio(hz, ratio):
    x, f0 = tracked_vowel(hz)
    n = len(x)
    per, rat = pr.tables(f0, 16000, ratio=ratio)
    y, _, _ = pr.shift(x, n, per, rat, 80)
    inside = f0_ref.fully_voiced_frames(np.ones(n, bool), 80, 512, f0_ref.lag_range(16000)[1])
    for name, got in (('yin', f0_ref.yin(y)[0]), ('viterbi', f0_track_ref.track(y)[0])):
        keep = inside & (got > 0)
        assert keep.sum() >= 80
        c = float(f0_ref.cents(np.median(got[keep]), hz * ratio))
        print('%.0f Hz x %.2f, %s: %.2f cents over %d frames' % (hz, ratio, name, c, keep.sum()))
        if name == 'yin' or (hz, ratio) not in OCTAVE_LOW:
            assert abs(c) <= 20.0, (name, c)


def test_formants_stay_where_they_were():
    """Energy per 500 Hz band below 3 kHz, before and after a shift: within 6 dB (the harmonics sample the same envelope at
    other frequencies; the issue's prototype saw at most 4.3 dB)."""
    x, f0 = tracked_vowel(120.0)
    per, rat = pr.tables(f0, 16000, ratio=0.8)
    y, _, _ = pr.shift(x, len(x), per, rat, 80)
    band = lambda v: np.add.reduceat(np.abs(np.fft.rfft(v[1000:7000].astype(np.float64) * np.hanning(6000))) ** 2,
                                     np.arange(0, 3000 * 6000 // 16000, 500 * 6000 // 16000))
    d = 10 * np.log10(band(y) / band(x))
    assert np.abs(d).max() <= 6.0, d


# ------------------------------------------------------------------------------------------------ the host path of conversion.py
def test_pitch_tables_match_numpy_on_the_host():
    import conversion
    rng = np.random.RandomState(5)
    f0 = rng.uniform(60, 400, (3, 40)).astype(np.float32)
    f0[rng.rand(3, 40) < 0.3] = 0.0
    f0[0, 0], f0[0, 1] = 1e-30, 3e38                                 # periods beyond int32 and below one sample
    tgt = rng.uniform(60, 400, (3, 40)).astype(np.float32)
    tgt[rng.rand(3, 40) < 0.3] = 0.0
    per_frame = rng.uniform(0.5, 2.0, (3, 40))
    for kw in (dict(ratio=1.25), dict(ratio=per_frame), dict(target_f0=tgt)):
        for f in (f0, torch.from_numpy(f0)):
            per, rat = conversion.pitch_tables(f, 16000, unvoiced_period=64, **kw)
            wp, wr = pr.tables(f0, 16000, unvoiced_period=64, **kw)
            assert per.dtype == torch.int32 and rat.dtype == torch.int32 and per.device.type == 'cpu'
            assert np.array_equal(per.numpy(), wp) and np.array_equal(rat.numpy(), wr)
    per, _ = conversion.pitch_tables(f0, 16000, ratio=1.0, hop_length=100)
    assert (per.numpy()[f0 == 0] == 100 << 16).all()
    assert int(conversion.pitch_tables(np.full((1, 1), 100.0), 16000, ratio=1.0)[0]) == 160 << 16
    for bad in (dict(), dict(ratio=1.0, target_f0=tgt), dict(ratio=0.4), dict(ratio=2.5), dict(ratio=float('nan')), dict(ratio=True),
                dict(ratio=per_frame[:2]), dict(ratio=per_frame * 3), dict(target_f0=tgt[:, :5]), dict(ratio=1.0, unvoiced_period=0),
                dict(ratio=1.0, unvoiced_period=2.5)):
        with pytest.raises(ValueError):
            conversion.pitch_tables(f0, 16000, **bad)
    with pytest.raises(ValueError):
        conversion.pitch_tables(f0[0], 16000, ratio=1.0)
    with pytest.raises(ValueError):
        conversion.pitch_tables(f0, 0, ratio=1.0)
    assert np.array_equal(conversion.psola_window(), pr.window()) and pr.window()[0] == 1.0 and pr.window()[2048] == 0.0
    assert (np.diff(pr.window()) < 0).all()


def test_f0_stats_and_transform_match_numpy_on_the_host():
    import conversion
    rng = np.random.RandomState(6)
    f0 = rng.uniform(80, 300, (4, 50)).astype(np.float32)
    f0[rng.rand(4, 50) < 0.4] = 0.0
    nf = np.array([50, 31, 1, 0])
    keep = (f0 > 0) & (np.arange(50)[None] < nf[:, None])
    lf = np.log(f0[keep].astype(np.float64))
    for n_frames in (nf, torch.from_numpy(nf), nf.tolist()):
        st = conversion.f0_stats_batch(f0, n_frames)
        assert int(st.count) == keep.sum() and abs(float(st.mean) - lf.mean()) < 1e-12 and abs(float(st.std) - lf.std()) < 1e-12
    allf = conversion.f0_stats_batch(torch.from_numpy(f0))
    assert int(allf.count) == (f0 > 0).sum()
    none = conversion.f0_stats_batch(np.zeros((2, 5), np.float32))
    assert int(none.count) == 0 and float(none.mean) == 0.0 and float(none.std) == 0.0
    with pytest.raises(ValueError):
        conversion.f0_stats_batch(f0[0])
    with pytest.raises(ValueError):
        conversion.f0_stats_batch(f0, [1, 2])
    src, tgt = (10, 5.0, 0.2), (12, 5.5, 0.3)
    got = conversion.f0_transform(f0, src, tgt).numpy()
    want = np.where(f0 > 0, np.exp((np.log(np.where(f0 > 0, f0, 1).astype(np.float64)) - 5.0) * 1.5 + 5.5), 0.0).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got == 0, f0 == 0) and np.allclose(got, want, rtol=1e-6, atol=0)
    # a source without spread: moved by the means alone; the statistics of f0_stats_batch go in as they come out
    flat = conversion.f0_transform(f0, (3, 5.0, 0.0), tgt).numpy()
    assert np.allclose(flat[f0 > 0], (f0[f0 > 0].astype(np.float64) * np.exp(0.5)).astype(np.float32), rtol=1e-6)
    same = conversion.f0_transform(torch.from_numpy(f0), st, st).numpy()
    assert np.allclose(same, f0, rtol=1e-6)
    with pytest.raises(ValueError):
        conversion.f0_transform(f0, (5.0, 0.2), tgt)
