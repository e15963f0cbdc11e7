"""The cases of tests/score_kernels_cases.py are usable, without a device: the exact DTW cases have integer costs and real
ties, the YIN configurations reach every tile size and every lane count they name, the float64 reference alone keeps its
marginal frames under the cap on every signal, the tie case ties, the mask patterns hold the runs they promise; and the
additive extensions of the references agree with what they extend.  The bound functions live in score_kernels_cases.py
and are pinned here."""
import numpy as np
import pytest

import activity_ref as ar
import f0_ref as fr
import f0_track_ref as tr
import mcd_ref as mr
import score_kernels_cases as Cs


# ------------------------------------------------------------------------------------------------ DTW
def test_dtw_tables_hold_what_the_issue_names():
    pairs = [p for _, ps in Cs.DTW_EXACT for p in ps]
    assert {(1025, 513), (2049, 257), (1024, 512)} <= set(pairs)
    assert {a for a, _ in pairs} <= {1, 3, 4, 5, 1023, 1024, 1025, 2049}
    assert {b for _, b in pairs} <= {1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025}
    assert [n for n, _ in Cs.DTW_EXACT] == [1, 8, 9, 16, 17, 24, 25, 32]


@pytest.mark.parametrize('n_coef', [n for n, _ in Cs.DTW_EXACT])
def test_exact_dtw_cases_have_integer_costs_and_ties(n_coef):
    for k, (a, b) in enumerate(Cs.dtw_exact_pairs(n_coef)):
        assert a.shape[1] == b.shape[1] == n_coef
        if n_coef > 1:
            d = mr.dist(a[:, None, :][:8], b[None, :64, :])
            assert np.array_equal(d, np.round(d)), (n_coef, k)
            d32 = mr.dist(a[:, None, :][:8], b[None, :64, :], dtype=np.float32)
            assert np.array_equal(d32.astype(np.float64), d)
        if len(a) >= 16 and len(b) >= 16:
            assert (a[:-1, 0] == a[1:, 0]).any() and (a[:-1, 0] != a[1:, 0]).any()       # equal and unequal neighbours


def test_dtw_loop_and_dtw_agree_and_define_the_unreachable_end():
    rng = np.random.RandomState(0)
    a, b = Cs.int_cepstra(rng, 9, 9), Cs.int_cepstra(rng, 14, 9)
    for band in (None, 3, 1, 0):
        t0, n0, p0 = mr.dtw_loop(a, b, 1.0, band)
        t1, n1, p1 = mr.dtw(a, b, 1.0, band)
        assert t0 == t1 and n0 == n1 and ((p0 is None and p1 is None) or np.array_equal(p0, p1)), band
    assert not np.isfinite(mr.dtw(a, b, 1.0, 0)[0]) and mr.dtw(a, b, 1.0, 0)[2] is None
    assert np.isfinite(mr.dtw(a, a, 1.0, 0)[0])                                            # Fa == Fb: the diagonal is inside


def test_band_cases_are_what_they_claim():
    for n_coef, (Fa, Fb) in Cs.DTW_BAND:
        a, b, free, need = Cs.dtw_band_pair(n_coef, Fa, Fb)
        assert need >= 1
        wide = Cs.dtw_band_reference(n_coef, Fa, Fb, need)
        assert wide[0] == free[0] and np.array_equal(wide[2], free[2])
        narrow = Cs.dtw_band_reference(n_coef, Fa, Fb, need - 1)
        assert narrow[0] >= free[0] and (narrow[2] is None or not np.array_equal(narrow[2], free[2]))
        if Fa != Fb:
            assert not np.isfinite(Cs.dtw_band_reference(n_coef, Fa, Fb, 0)[0])


def test_bounds_are_the_formulas():
    assert Cs.dtw_real_bound(257, 300, 24) == 2.0 * (257 + 300 + 24 + 2) * 2.0 ** -24
    assert abs(Cs.frame_mcd_bound(513, 13) / ((13 + 3 + 3 + 8 + 1) * Cs.EPS) - 1) < 1e-5
    assert abs(Cs.energy_bound(8192) / ((128 + 6) * Cs.EPS) - 1) < 1e-4 and abs(Cs.energy_bound(1) / (7 * Cs.EPS) - 1) < 1e-5
    assert Cs.gain_bound() < 2.0 * Cs.EPS
    assert Cs.metrics_bound(100.0, 1000) < 1.01 * float(np.spacing(np.float32(100.0)))
    tab, mel = np.ones((2, 5), np.float32), np.full((3, 5), 2.0, np.float32)
    assert np.allclose(Cs.cepstra_bound(tab, mel), 10.0 * 5 * Cs.EPS, rtol=1e-5)
    assert {min(p) for p in Cs.FRAME_MCD_PAIRS} == {1, 255, 256, 257, 513}
    assert Cs.CEPSTRA_LONG[0] * Cs.CEPSTRA_LONG[2] > 4096 * 256 and 512 * 32 * 4 == Cs.LDS_BUDGET


# ------------------------------------------------------------------------------------------------ YIN
def test_yin_configurations_reach_every_tile_size_and_lane_count():
    tiles = {}
    for name, (W, hop, tau_min, tau_max) in Cs.YIN_CONFIGS.items():
        G = Cs.yin_tile(W, tau_max, hop)
        assert G == Cs.yin_tile(W, tau_max, hop, cand=True), name            # the two kernels tile these cases alike
        assert G == Cs.YIN_TILES.get(name, 16), (name, G)
        assert Cs.yin_lds_bytes(W, tau_max, hop, G, cand=True) <= Cs.LDS_BUDGET
        assert 1 <= tau_min <= tau_max <= 1022 and W <= 2048
        tiles[G] = tiles.get(G, 0) + 1
        lens = Cs.yin_lengths(name)
        assert {0, 1, hop - 1, hop, G * hop - 1, G * hop, G * hop + 1} <= set(lens) and max(lens) > G * hop + 1
    assert set(tiles) == {16, 8, 4, 2, 1}
    assert Cs.yin_lanes(62) == 64 and Cs.yin_lanes(63) == 128 and Cs.yin_lanes(1022) == 1024
    assert Cs.yin_lds_bytes(2048, 1022, 256, 16, cand=True) <= Cs.LDS_BUDGET
    assert {c[0] for c in Cs.YIN_CONFIGS.values()} >= {1, 7, 8, 9, 2048}
    assert any(c[2] == c[3] for c in Cs.YIN_CONFIGS.values()) and any(c[2] == 1 for c in Cs.YIN_CONFIGS.values())
    assert set(Cs.YIN_NCAND.values()) == {1, 2, 15}
    assert 1 + max(Cs.yin_lengths('shipped')) // 80 >= 100


@pytest.mark.parametrize('name', list(Cs.YIN_CONFIGS))
def test_the_reference_alone_keeps_its_marginal_frames_under_the_cap(name):
    """The cap is a condition on the signals: at most 1 % of a row of 100 frames or more, none of a shorter row, in
    the float64 definition itself; and the rows are not trivially unvoiced."""
    voiced = 0
    for b, ((f0, ap, det), _) in enumerate(Cs.yin_reference(name)):
        F = len(f0)
        assert det['marginal'].sum() <= (0.01 * F if F >= 100 else 0), (name, b, F, np.nonzero(det['marginal'])[0])
        voiced += int((f0 > 0).sum())
    assert voiced > 0, name
    # the candidates' marginal frames (f0_track_ref.marginal_frames: a flag or a rank within float32's reach, exact ties at
    # the zero-padded ends among them) are left out of the device comparison; most frames must remain, some with candidates
    sure = [(~c64['marginal']) for c64, _ in Cs.cand_reference(name)]
    n_sure, n_all = sum(int(m.sum()) for m in sure), sum(len(m) for m in sure)
    assert n_sure >= 0.6 * n_all, (name, n_sure, n_all)
    assert sum(int(c64['n'][m].sum()) for (c64, _), m in zip(Cs.cand_reference(name), sure)) > 0, name


def test_yin_with_a_lag_range_is_yin_with_the_frequencies_that_give_it():
    x = fr.glide_signal(11)[0][:4000]
    a = fr.yin(x)
    b = fr.yin(x, tau_min=40, tau_max=267)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = fr.candidates(x, 16000, 80, 512, 40, 267, 8, 1.0)
    d = tr.candidates(x)
    for k in ('lag', 'f0', 'pitch', 'cost', 'n', 'aperiodicity', 'marginal'):
        assert np.array_equal(c[k], d[k]), k


def test_candidate_cases_are_what_they_claim():
    for n_cand in (1, 2, 15):
        c = Cs.many_minima_reference(n_cand)
        r = c['dp'][:, Cs.MANY['tau_min']:Cs.MANY['tau_max'] + 1]
        inner = (r[:, 1:-1] < r[:, :-2]) & (r[:, 1:-1] <= r[:, 2:])
        assert (inner[Cs.MANY_KEEP].sum(1) > 15).all()                                                  # more local minima than any n_cand
        assert (c['n'][Cs.MANY_KEEP] == n_cand).all() and not c['marginal'][Cs.MANY_KEEP].any()
    # the tie: d' is exactly zero at every multiple of the period on the interior frames, in both precisions
    t = Cs.TIE
    x = Cs.tie_signal()
    keep = Cs.tie_interior_frames()
    assert len(keep) >= 10
    for dtype in (np.float64, np.float32):
        dp, _ = fr.dprime(x, t['hop'], t['W'], t['tau_max'], dtype)
        assert (dp[keep][:, [12, 24, 36]] == 0).all() and (dp[keep][:, [11, 13, 23, 25]] > 0).all()
        c = fr.candidates(x, Cs.SR, t['hop'], t['W'], t['tau_min'], t['tau_max'], 2, 1.0, dtype)
        assert (c['lag'][keep] == [12, 24]).all() and (c['cost'][keep] == 0).all()
    # the plateau: lag 1 ties with lag 2; only the left one of the pair is a candidate, in either precision
    c = Cs.PLATEAU
    for dtype in (np.float64, np.float32):
        ref = fr.candidates(Cs.plateau_signal(), Cs.SR, c['hop'], c['W'], c['tau_min'], c['tau_max'], c['n_cand'], c['ceiling'], dtype)
        assert ref['dp'][c['frame'], 1] == ref['dp'][c['frame'], 2] == 1 and ref['dp'][c['frame'], 4] == 0
        assert ref['n'][c['frame']] == 3 and tuple(ref['lag'][c['frame']]) == c['lags']
    # a ceiling below every d' of a whole tone: no candidate anywhere
    for name in Cs.NO_CAND_CONFIGS:
        c64 = Cs.cand_reference(name)[-1][0]
        assert c64['aperiodicity'].min() > 10 * Cs.NO_CAND_CEILING, (name, c64['aperiodicity'].min())


# ------------------------------------------------------------------------------------------------ energy, masks
def test_energy_configurations_reach_the_tiles_named():
    assert [Cs.energy_tile(W, hop) for W, hop in Cs.ENERGY_CONFIGS] == Cs.ENERGY_TILES
    assert {W for W, _ in Cs.ENERGY_CONFIGS} == {1, 63, 64, 65, 400, 8192}
    for W, hop in Cs.ENERGY_CONFIGS:
        rows = Cs.energy_rows(W, hop)
        e64, e32 = ar.frame_energy(rows[-1], hop, W), ar.frame_energy(rows[-1], hop, W, np.float32)
        assert (np.abs(e32 - e64) <= Cs.energy_bound(W) * e64).all(), (W, hop)         # the restatement meets the bound


def test_mask_patterns_hold_the_runs_they_promise():
    assert [Cs.chunk(F) for F in Cs.MASK_FRAMES] == [1, 1, 1, 1, 2, 2, 3, 16]
    for F in Cs.MASK_FRAMES[2:]:
        for m in (Cs.lane_pattern(F), Cs.mirrored(Cs.lane_pattern(F))):
            runs = ar.runs(m)
            C = Cs.chunk(F)
            gaps = {e - s for v, s, e in runs if not v and s > 0 and e < F and (s // C != (e - 1) // C)}
            acts = {e - s for v, s, e in runs if v and (s // C != (e - 1) // C or C == 1)}
            assert {Cs.MAX_GAP, Cs.MAX_GAP + 1} <= gaps, (F, gaps)
            assert {Cs.MIN_RUN - 1, Cs.MIN_RUN} <= acts, (F, acts)
            ends = {(runs[0][0], runs[0][2] - runs[0][1]), (runs[-1][0], runs[-1][2] - runs[-1][1])}
            assert ends == {(True, Cs.MIN_RUN), (True, Cs.MIN_RUN - 1)}, (F, ends)
            out = ar.smooth(m, Cs.MAX_GAP, Cs.MIN_RUN)
            assert (out != m).any()
        rng = np.random.RandomState(F)
        raw = Cs.lane_pattern(F)
        assert np.array_equal(Cs.raw_decision(Cs.energies_of(raw, rng), 1e-4), raw)
    assert not Cs.raw_decision(np.array([1.0, 0.25], np.float32), 0.25)[1]                 # equal to the threshold: inactive
    assert Cs.raw_decision(np.array([1.0, np.nextafter(np.float32(0.25), np.float32(1))], np.float32), 0.25)[1]


def test_sample_to_frame_map_at_its_seams():
    for hop in Cs.GAIN_HOPS:
        F = 5
        i = np.arange(6 * hop)
        f = Cs.frame_of_sample(i, hop, F)
        assert f[0] == 0 and f[hop - hop // 2 - 1] == 0 and f[hop - hop // 2] == 1 and f[-1] == F - 1
        x = np.ones(len(i), np.float32)
        m = np.zeros(F, bool)
        m[1] = True
        assert ar.speech_gain(x, m, hop, 1.0) == 1.0
        assert (f == 1).sum() == hop
