"""Waveform time scaling, host side (include/vc_hip.h, "Time scale"): the numpy restatement of
tests/wsola_ref.py against facts that do not go through it, and the argument checks of conversion.time_scale_batch,
wsola_plan_batch and convert_diff_duration_batch, which all fail before anything touches a GPU.  No GPU."""
import numpy as np
import pytest

import diff_ref
import f0_ref
import wsola_ref as wr

Q = wr.Q
HOP, G, TOL = 8, 2, 12
S = HOP * G


def inner_map(rng, n_out, rate, hop=HOP, S=S, tol=TOL, jitter=0.0):
    """(pos [n_out], len): a monotone map of ``rate`` output frames per input frame (with ``jitter``, steps that vary by
    that fraction) whose targets keep every grain and every candidate inside [0, len): the first target lies S + tol
    samples in (rounded up to frames), the input ends 2 S + tol samples after the last."""
    f0 = -(-(S + tol) // hop) + 1
    step = np.full(n_out, 1.0 / rate)
    if jitter:
        step = step * rng.uniform(1.0 - jitter, 1.0 + jitter, n_out)
    fr = f0 + np.concatenate([[0.0], np.cumsum(step[:-1])])
    pos = np.rint(fr * Q).astype(np.int64)
    n = int((pos[-1] * hop + 32768) >> 16) + 2 * S + tol + 1
    return pos.astype(np.int32), n


def periodic(rng, P, n):
    base = rng.uniform(-0.9, 0.9, P).astype(np.float32)
    return base[np.arange(n) % P]


def test_the_identity_map_returns_noise_bit_for_bit():
    """d = 0 costs 0 at every grain whose target is k * S.  The LAST grain's frame is cut at n_out - 1, so where g does not
    divide n_out - 1 its target lies (K - 1) * S - out_len < S samples short of the continuation: the search finds it
    when tol reaches that far (the default does), and the cases with a smaller tol here have g | n_out - 1."""
    rng = np.random.RandomState(1)
    for hop, g, n_fr, tol in ((8, 2, 40, None), (80, 2, 12, None), (5, 3, 34, 0), (8, 1, 50, 3), (8, 4, 39, 25)):
        n = hop * n_fr + 3 * hop * g                                # the input goes on beyond the map
        x = rng.standard_normal(n).astype(np.float32) * 0.3
        y, p = wr.scale(x, n, wr.identity_map(n_fr), n_fr, hop, g, tol)
        assert p.out_len == hop * (n_fr - 1) and p.a[:p.K].tolist() == [k * hop * g for k in range(p.K)]
        assert (p.cost[:p.K] == 0).all()
        assert np.array_equal(y.view(np.int32), x[:p.out_len].view(np.int32))


RATES = (0.5, 0.6, 1.37, 2.0)


@pytest.mark.parametrize('P', [7, 13, 25])
def test_a_periodic_signal_comes_back_as_its_periodic_extension_at_any_rate(P):
    """P <= 2 tol + 1: some candidate continues the previous grain exactly, whatever the map."""
    rng = np.random.RandomState(P)
    for rate, jitter in [(r, 0.0) for r in RATES] + [(0.9, 0.6)]:
        pos, n = inner_map(rng, 60, rate, jitter=jitter)
        x = periodic(rng, P, n)
        y, p = wr.scale(x, n, pos, len(pos), HOP, G, TOL)
        assert p.out_len == HOP * 59 and (p.cost[:p.K] == 0).all()
        want = x[(np.arange(p.out_len) + int(p.a[0])) % P]
        assert np.array_equal(y.view(np.int32), want.view(np.int32)), (P, rate)
        assert (np.abs(p.a[:p.K] - np.array(p.tau)) <= TOL).all()


@pytest.mark.parametrize('P,tol,rates', [(26, TOL, (16.0 / 29.0, 16.0 / 3.0)), (13, 0, RATES)])
def test_without_a_wide_enough_search_the_extension_fails(P, tol, rates):
    """The same signal family one sample of period beyond the search (P = 2 tol + 2), and with no search at all: the
    output is NOT the periodic extension -- so the property above is the search's doing.  With P = 26 the search still
    holds 25 of the 26 phases, so a map defeats it only where a step asks for the one it lacks, d = +-13: a uniform map that
    moves 29 (or 3) input samples per grain of 16 asks for it at the first step, and the phase is lost from there on.  (At
    the rates of the test above every step of a uniform map asks for the same offset, and for none of them is it 13.)"""
    rng = np.random.RandomState(P + tol)
    for rate in rates:
        pos, n = inner_map(rng, 60, rate, tol=TOL)
        x = periodic(rng, P, n)
        y, p = wr.scale(x, n, pos, len(pos), HOP, G, tol)
        want = x[(np.arange(p.out_len) + int(p.a[0])) % P]
        bad = np.mean(y[S:] != want[S:])                            # (the first S samples are grain 0 alone where B has weight ~0)
        print('P %d tol %d rate %.2f: %.1f %% of the samples differ' % (P, tol, rate, 100 * bad))
        assert bad > 0.5, (P, tol, rate, bad)


def test_the_positions_stay_within_tol_of_the_map_on_junk():
    rng = np.random.RandomState(5)
    for trial in range(12):
        hop, g = int(rng.choice([1, 3, 8])), int(rng.choice([1, 2, 4]))
        tol = int(rng.choice([0, 1, 7, 20]))
        F = int(rng.randint(1, 40))
        n = int(rng.randint(1, 300))
        x = rng.standard_normal(n + 5).astype(np.float32)
        pos = rng.randint(-2 ** 31, 2 ** 31, F).astype(np.int64).astype(np.int32)
        near = rng.rand(F) < 0.5
        pos[near] = rng.randint(0, (n // hop + 2) << 16, int(near.sum()))
        n_out = int(rng.randint(0, F + 1))
        p = wr.plan(x, n, pos, n_out, hop, g, tol)
        assert (p.out_len, p.K) == wr.sizes(n_out, n, hop, hop * g)
        if p.K:
            tau = np.array(p.tau)
            assert tau.min() >= 0 and tau.max() <= n - 1
            assert (np.abs(p.a[:p.K].astype(np.int64) - tau) <= tol).all() and p.a[0] == tau[0] and p.cost[0] == 0
        assert (p.a[p.K:] == -2 ** 31).all() and (p.cost[p.K:] == -1).all() and len(p.a) == wr.max_grains(F, hop, hop * g)


@pytest.mark.parametrize('value', [0.0, 0.37])
def test_a_tie_takes_d_zero(value):
    """All-zero and constant signals: every candidate that stays inside the signal costs the same, and the rule
    (cost, |d|, d) takes d = 0 at every step."""
    n = 2000
    x = np.full(n, value, np.float32)
    rng = np.random.RandomState(6)
    pos, _ = inner_map(rng, 50, 1.3, jitter=0.4)
    assert ((int(pos[-1]) * HOP) >> 16) + 2 * S + TOL < n
    p = wr.plan(x, n, pos, len(pos), HOP, G, TOL)
    assert p.a[:p.K].tolist() == list(p.tau) and (p.cost[:p.K] == 0).all()


def test_the_tie_rule_prefers_the_smaller_then_the_negative_offset():
    """Period 4 and tol 3: offsets one period apart cost the same; of -1 and +3 the nearer, of -2 and +2 the negative."""
    n, hop, g = 400, 4, 1
    x = np.tile(np.array([0.1, 0.5, -0.3, 0.2], np.float32), n // 4)
    for shift, want in ((1, -1), (3, 1), (2, -2)):
        # grain 0 at sample 40, the target of grain 1 at 44 + shift: the continuation 44 lies at d = -shift (and +4 - shift)
        pos = np.array([10 << 16, ((44 + shift) << 16) // hop], np.int32)
        p = wr.plan(x, n, pos, 2, hop, g, 3)
        assert p.K == 2 and p.tau == [40, 44 + shift]
        assert int(p.a[1]) - p.tau[1] == want and p.cost[1] == 0, (shift, p.a[:2], want)


def test_quantisation_of_specials_and_clipping():
    x = np.array([0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 0.99999, 3.0, -3.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768,
                  1e-30, 3e38], np.float32)
    assert wr.quantise(x).tolist() == [0, 0, 32767, -32767, 32767, -32767, 32767, 32767, -32767, 0, 2, 2, 0, 0, 32767]
    assert wr.quantise(x, 3e38).tolist()[4:8] == [32767, -32767, 32767, 32767]
    assert wr.quantise(np.array([0.26, -0.26], np.float32), 10.0).tolist() == [3, -3]


def test_sizes_against_the_closed_forms_and_short_inputs():
    x = np.linspace(-1, 1, 64).astype(np.float32)
    for n_out, n, want in ((0, 64, (0, 0)), (1, 64, (0, 0)), (2, 64, (8, 2)), (2, 0, (0, 0)), (5, 1, (32, 3)), (4, 64, (24, 3))):
        pos = wr.identity_map(8)
        p = wr.plan(x, n, pos, n_out, 8, 2)
        assert (p.out_len, p.K) == want == wr.sizes(n_out, n, 8, 16), (n_out, n)
        y = wr.ola(x, n, p.a, p.K, p.out_len, 16, 8 * 7)
        assert not y[p.out_len:].any()
        if n == 1:                                                  # one sample: every target is sample 0
            assert p.tau == [0, 0, 0]
    for F, hop, g in ((1, 8, 2), (2, 8, 2), (3, 8, 2), (100, 80, 2), (16384, 1024, 1), (7, 5, 3)):
        assert wr.max_grains(F, hop, hop * g) == wr.sizes(F, 1, hop, hop * g)[1] or F == 1
    assert wr.max_grains(1, 8, 16) == 1


def test_the_last_grains_target_is_the_last_frame():
    """g * k beyond n_out - 1: u_k stops at the last frame of the map."""
    pos = (np.arange(6, dtype=np.int64) * 3 << 16).astype(np.int32)            # frames 0, 3, ..., 15
    x = np.random.RandomState(7).standard_normal(400).astype(np.float32)
    p = wr.plan(x, 400, pos, 6, 8, 4, 0)                                       # S = 32, out_len = 40, K = 3: u = 0, 4, 5
    assert p.K == 3 and p.tau == [0, 12 * 8, 15 * 8]


def test_the_window_and_the_overlap_add_of_a_hand_made_plan():
    T = wr.window(16)
    assert T[0] == 0.0 and T.dtype == np.float32 and abs(T[8] - 0.5) < 1e-7 and (np.diff(T) > 0).all()
    x = np.arange(1, 101, dtype=np.float32)
    a = np.array([10, 50, 2 ** 24 + 1, 0], np.int32)
    y = wr.ola(x, 100, a, 3, 40, 16, 48)
    r = np.arange(16)
    lerp = lambda A, B: A + (T * (B - A).astype(np.float32)).astype(np.float32)
    assert np.array_equal(y[:16], lerp(x[10 + r], x[50 + r - 16]))
    assert np.array_equal(y[16:32], lerp(x[50 + r], np.zeros(16, np.float32)))         # grain 2 is beyond the guard
    assert np.array_equal(y[32:40], np.zeros(8, np.float32)) and not y[40:].any()      # grain 3 is beyond n_grains


# ------------------------------------------------------------------------------------------------ two synthetic vowels
# Measured on the restatement (float32) at the defaults (hop 80, group 2, tol 160), printed by the tests below and recorded
# in DESIGN.md section 27.
VOWELS = {'a': (110.0, diff_ref.VOWEL_A), 'i': (190.0, diff_ref.VOWEL_I)}
_vowel = {}


def vowel(name, n=12000):
    if name not in _vowel:
        hz, form = VOWELS[name]
        _vowel[name] = diff_ref.vowel(diff_ref.pulse_train(np.full(n, hz)), *form).astype(np.float32)
    return _vowel[name]


_stretched = {}


def stretched(name, rate):
    if (name, rate) not in _stretched:
        x = vowel(name)
        pos, Lo = wr.rate_map(1 + len(x) // 80, rate)
        _stretched[(name, rate)] = wr.scale(x, len(x), pos, Lo, 80)
    return _stretched[(name, rate)]


@pytest.mark.parametrize('name', ['a', 'i'])
@pytest.mark.parametrize('rate', [0.7, 1.5])
def test_a_stretched_vowel_keeps_its_fundamental(name, rate):
    y, p = stretched(name, rate)
    hz = VOWELS[name][0]
    assert abs(p.out_len - rate * len(vowel(name))) <= 80
    f0 = f0_ref.yin(y[:p.out_len])[0]
    inside = f0_ref.fully_voiced_frames(np.ones(p.out_len, bool), 80, 512, f0_ref.lag_range(16000)[1])
    keep = inside & (f0 > 0)
    assert keep.sum() >= 50
    c = f0_ref.cents(f0[keep], hz)
    print('/%s/ %.0f Hz x %.1f: median %.2f cents, worst frame %.2f cents over %d frames' % (name, hz, rate, float(np.median(c)),
                                                                                         float(np.abs(c).max()), keep.sum()))
    assert abs(float(f0_ref.cents(np.median(f0[keep]), hz))) <= 20.0


@pytest.mark.parametrize('name', ['a', 'i'])
@pytest.mark.parametrize('rate', [0.7, 1.5])
def test_a_stretched_vowel_keeps_its_formants(name, rate):
    """Energy per 500 Hz band below 3 kHz, before and after: within 6 dB, the cap of the pitch tests."""
    y, p = stretched(name, rate)
    band = lambda v: np.add.reduceat(np.abs(np.fft.rfft(v[1000:7000].astype(np.float64) * np.hanning(6000))) ** 2,
                                     np.arange(0, 3000 * 6000 // 16000, 500 * 6000 // 16000))
    d = 10 * np.log10(band(y) / band(vowel(name)))
    print('/%s/ x %.1f: band energies move by %s dB' % (name, rate, np.round(d, 2).tolist()))
    assert np.abs(d).max() <= 6.0, d


# ------------------------------------------------------------------------------------------------ the host path of conversion.py
def test_the_window_of_the_package_is_the_restatements():
    import conversion
    for s in (1, 2, 16, 160, 1024):
        assert np.array_equal(conversion.wsola_window(s).view(np.int32), wr.window(s).view(np.int32))
    for bad in (0, 1025, 1.5, True):
        with pytest.raises(ValueError):
            conversion.wsola_window(bad)


def test_argument_checks_fail_before_any_launch():
    import conversion
    wav = np.zeros((2, 4000), np.float32)
    pos = np.zeros((2, 50), np.int32)
    ok = dict(wav=wav, lens=[4000, 3000], pos=pos, n_out=[50, 20], hop_length=80)
    bad = [dict(hop_length=0), dict(hop_length=1025), dict(hop_length=80.0), dict(group=0), dict(group=13), dict(hop_length=600, group=2),
           dict(tol=-1), dict(tol=1025), dict(tol=1.0), dict(qscale=0.0), dict(qscale=-1.0), dict(qscale=float('inf')),
           dict(qscale=float('nan')), dict(qscale=1e-60), dict(wav=wav[0]), dict(wav=wav.astype(np.float64)[:, :0]),
           dict(pos=pos[:1]), dict(pos=pos[0]), dict(pos=pos.astype(np.float32)), dict(lens=[4001, 1]), dict(lens=[-1, 1]),
           dict(lens=[1, 2, 3]), dict(n_out=[51, 1]), dict(n_out=[-1, 1]), dict(n_out=[1.0, 2.0]),
           dict(pos=np.zeros((2, 16385), np.int32), n_out=[1, 1])]
    for fn in (conversion.time_scale_batch, conversion.wsola_plan_batch):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(**dict(ok, **kw))
    import torch
    with pytest.raises(ValueError):
        conversion.time_scale_batch(**dict(ok, wav=torch.zeros((2, 4000), dtype=torch.float64)))
    for kw in (dict(), dict(rate=1.0, ratio=[1.0]), dict(rate=1.0, out_len=np.zeros((1, 1), np.int32)), dict(rate=0.0), dict(rate=9.0),
               dict(rate=True), dict(rate=1.0, gap_ratio=-1.0), dict(ratio=[1.0], segments='viterbi'), dict(rate=1.0, decode={}),
               dict(ratio=[1.0], decode=dict(no_such=1))):
        with pytest.raises(ValueError):
            conversion.convert_diff_duration_batch(None, wav, cfg_d={}, **kw)
    with pytest.raises(ValueError):
        conversion.convert_diff_duration_batch(None, wav, rate=1.0)
