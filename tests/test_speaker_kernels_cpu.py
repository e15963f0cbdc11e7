"""The cases of tests/speaker_kernels_cases.py are usable, without a device: every wrap case has a partition that takes two
or more tiles of one utterance, every `b >= P` case has such an utterance, the M, D and G seams are the ones the table
names, every exact case is exact in the float64 reference (integer sums, gamma 0 or 1), every bound holds the float32
restatement's own error on its case, and no frame is left out of any comparison.  The bound functions live in
speaker_kernels_cases.py and are pinned here; the additive extensions of tests/speaker_ref.py agree with what they extend."""
import fractions

import numpy as np
import pytest

import speaker_kernels_cases as Cs
import speaker_ref as sr


# ------------------------------------------------------------------------------------------------ geometry
def test_partitions_and_workspace_are_the_header_formulas():
    assert [Cs.partitions(G) for G in (1, 2, 3, 4, 42, 43, 63, 64, 65, 127, 128, 4096)] == [128, 64, 42, 32, 3, 2, 2, 2, 1, 1, 1, 1]
    assert Cs.workspace_bytes(1, 256, 64) == 33820672 and Cs.workspace_bytes(65, 256, 64) == 0 and Cs.workspace_bytes(128, 1, 1) == 0
    assert Cs.workspace_bytes(3, 65, 48) == (3 * 42 * 2 * (64 * 97 + 1) * 8 + 255) // 256 * 256
    assert Cs.table_floats(2, 65, 48) == 3 * 65 * 48 + 65
    assert [Cs.table_floats(*s) for s in Cs.PREP_SHAPES[4:]] == Cs.PREP_SEAMS
    assert Cs.PREP_SHAPES[:4] == [(1, 1, 1), (2, 63, 3), (5, 65, 64), (1, 256, 64)]
    # the three index branches of the table and a last block that is partly filled
    for S, M, D in Cs.PREP_SHAPES:
        assert S * M * D >= 1 and M * D >= 1 and 1 <= M <= Cs.MAX_M and 1 <= D <= Cs.MAX_D
    assert any(Cs.table_floats(*s) % 256 for s in Cs.PREP_SHAPES) and any(Cs.table_floats(*s) % 256 == 0 for s in Cs.PREP_SHAPES)


def test_every_tile_is_walked_exactly_once():
    for name, c in Cs.ACC_EXACT.items():
        todo = Cs.walk(c['lens'], c['groups'], c['G'])
        seen = sorted(t for v in todo.values() for t in v)
        want = sorted((b, k) for b, n in enumerate(c['lens']) if 0 <= c['groups'][b] < c['G'] for k in range(Cs.n_tiles(n)))
        assert seen == want, name
        P = Cs.partitions(c['G'])
        for (g, p), v in todo.items():
            assert all(Cs.partition_of(b, k, P) == p and c['groups'][b] == g for b, k in v), name


def test_wrap_cases_wrap_and_b_ge_p_cases_have_such_an_utterance():
    named = {'wrap_p2': (64, 2, 65), 'wrap_p3': (42, 3, 129), 'wrap_p42': (3, 42, 1345), 'wrap_p128': (1, 128, 4097)}
    for name, (G, P, frames) in named.items():
        c = Cs.ACC_EXACT[name]
        assert c['G'] == G and Cs.partitions(G) == P and c['lens'] == [frames] and Cs.n_tiles(frames) > P, name
        assert Cs.wrapped(c['lens'], c['groups'], G) == [(0, k) for k in range(P, Cs.n_tiles(frames))], name      # the tiles `k += P` reaches
        assert (Cs.n_tiles(frames) == P + 1) == (name != 'wrap_p3'), name       # 129 frames are five tiles: two partitions step twice
    for name, c in Cs.ACC_EXACT.items():
        P = Cs.partitions(c['G'])
        w = Cs.wrapped(c['lens'], c['groups'], c['G'])
        assert bool(w and P > 1) == bool(c.get('wrap')), (name, w)            # (one partition takes every tile: no wrap to speak of)
        has = P > 1 and any(b >= P and 0 <= g < c['G'] and n > 0 for b, (n, g) in enumerate(zip(c['lens'], c['groups'])))
        assert has == bool(c.get('b_ge_p')), name
    c = Cs.ACC_EXACT['b_ge_p2']
    assert Cs.partitions(c['G']) == 2 and len(c['lens']) == 5 and (4, 2) in Cs.wrapped(c['lens'], c['groups'], c['G'])      # b >= P AND a second step
    c = Cs.ACC_EXACT['b_ge_p128']
    assert len(c['lens']) == 130 and set(c['lens']) == {1, 2, 3} and Cs.partitions(1) == 128
    for b in (128, 129):                                                          # b mod P with b >= P: partitions 0 and 1 again
        assert Cs.partition_of(b, 0, 128) == b - 128


def test_order_case_tells_the_documented_map_from_another():
    """The order case wraps, has tiles that (b + k) mod P and k mod P send to different partitions, and its ordered float64
    sum differs in bits from the same terms under the other map and from numpy's pairwise sum."""
    c = Cs.ORDER_CASE
    P = Cs.partitions(c['G'])
    assert P == 3 and Cs.wrapped(c['lens'], c['groups'], c['G']) == [(0, 3)]
    assert any(Cs.partition_of(b, k, P) != k % P for b, n in enumerate(c['lens']) for k in range(Cs.n_tiles(n)))
    rng = np.random.RandomState(0)
    B, F = len(c['lens']), max(c['lens'])
    # float32 values over many orders of magnitude, as responsibilities are: values of one magnitude would add exactly
    gamma = np.exp(-40.0 * rng.rand(B, F, c['M'])).astype(np.float32).astype(np.float64)
    keep = Cs.kept(c['lens'], F)
    got = Cs.ordered_sum(gamma, keep, c['lens'], c['groups'], c['G'])
    plain = np.zeros_like(got)
    for b, g in enumerate(c['groups']):
        plain[g] += gamma[b][keep[b]].sum(0)
    assert np.allclose(got, plain, rtol=1e-13, atol=0) and not np.array_equal(got, plain)
    shifted = Cs.ordered_sum(gamma, keep, c['lens'][::-1], c['groups'][::-1], c['G'])        # (another walk of other terms: differs at once)
    assert not np.array_equal(got, shifted)


def test_seams_are_what_the_table_says():
    assert Cs.ACC_PAIRS == ((64, 65), (127, 128))
    # 64 -> 65 is the switch from two partitions and a workspace to one partition writing the outputs; 127 and 128 are both
    # one partition, by the division 128 / 127 and by the compare G >= 128
    assert [Cs.partitions(G) for G in (64, 65, 127, 128)] == [2, 1, 1, 1]
    assert Cs.workspace_bytes(64, 65, 5) > 0 and not any(Cs.workspace_bytes(G, 65, 5) for G in (65, 127, 128))
    assert max(Cs.ACC_PAIR_CASE['groups']) == 63 and min(Cs.ACC_PAIR_CASE['groups']) == 0
    assert Cs.ACC_EXACT['z_limit']['G'] == Cs.MAX_G == 4096 and Cs.ACC_EXACT['z_limit']['shape'] == (1, 0, 1)
    assert {-1, 3, Cs.IFILL} <= set(Cs.ACC_EXACT['left_out']['groups']) and 1 not in Cs.ACC_EXACT['left_out']['groups']
    assert Cs.ACC_MS == (1, 64, 65, 256) and Cs.ACC_DS == (1, 4, 5, 63, 64)
    assert {-(-M // Cs.CHUNK) for M in Cs.ACC_MS} == {1, 2, 4} and {D % 4 for D in Cs.ACC_DS} == {0, 1, 3}
    assert {Cs.ACC_EXACT[k]['shape'][1] for k in Cs.ACC_EXACT} >= {0, 63, 64, 255}                     # the live components
    assert Cs.LL_MS == (1, 63, 64, 65, 128, 129, 192, 193, 255, 256) and Cs.LL_DS == (1, 63, 64) and Cs.LL_MODELS == (1, 2, 5)
    assert Cs.LL_LENS == [0, 1, 7, 8, 9, 31, 32, 33, 70] and Cs.LL_FRAMES == (33, 70)
    for S in Cs.LL_MODELS:
        raw, eff = Cs.ll_model_index(S)
        assert {-3, 0, S - 1, S + 5} == set(raw) and set(eff) == {0, S - 1}
    assert Cs.SCORE_LENS == [0, 1, 255, 256, 257, 513] and -(-513 // Cs.LANES) == 3
    assert Cs.FEAT_LENS == [-5, 0, 1, 2, 3, 4, 5, 257, 360] and Cs.FEAT_FRAMES == 260 and Cs.FEAT_COEF == (1, 31, 32)
    assert [f % 4 for f in Cs.ONE_KEPT] == [0, 1, 2, 3]
    assert [M * D for M, D in Cs.UPDATE_EM_SHAPES] == [255, 256, 258, 256 * 64]
    G, M, D = Cs.UPDATE_MAP_257
    assert G * M * D == 257 and all(257 % k for k in range(2, 257))


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize('name', list(Cs.ACC_EXACT) + ['pair'])
def test_exact_cases_are_exact_in_the_float64_reference(name):
    """gamma is 0 or 1 and the sums are the integers the case holds, in float64 and in the float32 restatement alike; the
    stored ll is float32(c - q / 2)."""
    c = Cs.acc_exact(name, 64 if name == 'pair' else None)
    assert np.array_equal(c['N'], np.round(c['N'])) and c['N'].sum() == sum(
        int(c['keep'][b].sum()) for b, g in enumerate(c['groups']) if 0 <= g < c['G'])
    assert c['N'].sum() > 0 and np.isnan(c['x'][0, Cs.feat_eff(c['lens'][0], c['F']):]).all()
    if c['mask'] is not None:
        assert (~c['keep'] & Cs.kept(c['lens'], c['F'])).any()                  # the mask drops a frame below a length
    with np.errstate(divide='ignore'):
        for dtype in (np.float64, np.float32):
            st = sr.accumulate(Cs.clean(c['x']), c['lens'], c['groups'], c['G'], c['w'], c['mu'][c['model']], c['var'], c['mask'], dtype)
            for k in ('N', 'S1', 'S2'):
                assert np.array_equal(st[k], c[k]), (name, k, dtype)
        cm = sr.log_norm(c['w'], c['var'])
        assert np.isneginf(np.delete(cm, c['m_star'])).all() and np.isfinite(cm[c['m_star']])
        b = int(np.argmax(c['lens']))
        n = c['lens'][b]
        ll32 = sr.loglik(c['x'][b, :n], c['w'], c['mu'][c['model']], c['var'], np.float32)[0]
    assert np.array_equal(ll32, Cs.exact_ll(cm[c['m_star']], c['x'][b, :n], c['mu'][c['model'], c['m_star']]))
    if c['S'] > 1:                                                               # another model's means give another ll
        other = Cs.exact_ll(cm[c['m_star']], c['x'][b, :n], c['mu'][(c['model'] + 1) % c['S'], c['m_star']])
        assert (other != ll32).any()


def test_issue_exact_values():
    """(M, m*, D, F) = (1, 0, 2, 4097), (65, 64, 3, 1345), (256, 255, 1, 130) of the issue, by shape."""
    got = {(c['shape'][0], c['shape'][1], c['shape'][2], sum(c['lens'])) for c in Cs.ACC_EXACT.values()}
    assert (65, 64, 3, 1345) in got and (2, 1, 2, 4097) in got
    assert Cs.ACC_EXACT['b_ge_p128']['shape'] == (256, 255, 1) and len(Cs.ACC_EXACT['b_ge_p128']['lens']) == 130


# ------------------------------------------------------------------------------------------------ bounds
def test_bounds_are_the_formulas():
    assert Cs.EPS == 2.0 ** -24 and Cs.U64 == 2.0 ** -53
    assert Cs.feat_bound(3.0) == 8.0 * 2.0 ** -24 * 3.0
    assert Cs.l_bound(4097) == 4097 * 2.0 ** -53
    assert Cs.order_bound(70, 2, 10.0) == 72 * 2.0 ** -53 * 10.0
    assert Cs.score_bound(-40.0, 513) == 0.5 * float(np.spacing(np.float32(40.0))) * (1 + 1e-6) + 513 * 2.0 ** -53 * 40.0
    assert Cs.score_bound(0.25, 10, 40.0) == 0.5 * float(np.spacing(np.float32(0.25))) * (1 + 1e-6) + 10 * 2.0 ** -53 * 40.0
    c, bound = Cs.c_reference(np.array([0.5, 0.0], np.float32), np.ones((2, 3), np.float32))
    t = np.log(2 * np.pi)
    assert c[0] == np.log(0.5) - 0.5 * (t + t + t) and np.isneginf(c[1])
    assert bound[0] == 0.5 * float(np.spacing(np.float32(abs(c[0])))) * (1 + 1e-6) + 5 * 2.0 ** -53 * (np.log(2.0) + 3 * t)
    assert Cs.UPDATE_ULPS == 2.0
    n, S1, S2 = Cs.cancellation_case()
    true, bound = Cs.cancellation_bound(n, S1, S2)
    F = fractions.Fraction
    assert bound == 0.5 * float(np.spacing(np.float32(true))) * (1 + 1e-6) + 4 * 2.0 ** -53 * float(F(S2) / F(n) + (F(S1) / F(n)) ** 2)
    assert sr.frame_bound(3, 4, 2.0) == (3 + 2 + 16.0) * 2.0 ** -24 * 2.0


def test_cancellation_case_cancels_and_float64_stays_inside_its_bound_fused_or_not():
    n, S1, S2 = Cs.cancellation_case()
    true, bound = Cs.cancellation_bound(n, S1, S2)
    assert 0 < true < 1e-8 * (S1 / n) ** 2
    for fused in (False, True):
        v = Cs.variance_float64(n, S1, S2, fused)
        assert abs(float(np.float32(v)) - true) <= bound, (fused, v, true, bound)
    assert Cs.variance_float64(n, S1, S2, False) != Cs.variance_float64(n, S1, S2, True)        # the two forms do differ here
    assert bound > 2.0 * float(np.spacing(np.float32(true)))          # ... by more than the benign cases' 2 ulp: hence a bound of its own


@pytest.mark.parametrize('D,M', [(8, 65), (64, 256), (1, 1), (63, 129)])
def test_loglik_bound_holds_the_float32_restatement(D, M):
    for F in Cs.LL_FRAMES:
        c = Cs.ll_case(D, M, 2, F)
        assert np.isnan(c['x'][1, 1:]).all() and np.isfinite(c['x'][8]).all()
        for b, n in enumerate(c['eff']):
            if n:
                want, E = sr.loglik(c['x'][b, :n], c['w'], c['mu'][1], c['var'])
                got = sr.loglik(c['x'][b, :n], c['w'], c['mu'][1], c['var'], np.float32)[0]
                assert (np.abs(got - want) <= sr.frame_bound(D, M, E)).all(), (D, M, b)


@pytest.mark.parametrize('D,M,G', Cs.ACC_REAL)
def test_accumulate_two_delta_rule_holds_the_float32_restatement(D, M, G):
    c = Cs.real_case(D, M)
    groups = [b % min(G, 3) if G > 1 else 0 for b in range(len(c['lens']))]
    x = Cs.clean(c['x'])
    want = sr.accumulate(x, c['lens'], groups, G, c['w'], c['mu'][0], c['var'], c['mask'])
    got = sr.accumulate(x, c['lens'], groups, G, c['w'], c['mu'][0], c['var'], c['mask'], np.float32)
    delta = max(float(bd.max()) for _, bd in Cs.real_ll(D, M))
    assert (np.abs(got['N'] - want['N']) <= 2 * delta * want['N'] + 1e-300).all()
    assert (np.abs(got['S1'] - want['S1']) <= 2 * delta * want['A1'] + 1e-300).all()
    assert (np.abs(got['S2'] - want['S2']) <= 2 * delta * want['S2'] + 1e-300).all()
    assert (np.abs(got['L'] - want['L']) <= delta * np.maximum(want['N'].sum(1), 1.0)).all()


# ------------------------------------------------------------------------------------------------ features, score, prepare
@pytest.mark.parametrize('n_coef', Cs.FEAT_COEF)
def test_features_restatement_extends_the_reference_and_meets_the_bound(n_coef):
    for deltas in (False, True):
        cep, mask = Cs.feat_batch(n_coef)
        icep, imask = Cs.feat_batch(n_coef, integer=True)
        for b, n in enumerate(Cs.FEAT_LENS):
            e = Cs.feat_eff(n)
            assert np.isnan(cep[b, e:]).all() and np.isfinite(cep[b, :e]).all() and (mask[b, e:] != 0).all()
            got = sr.features_f32(cep[b], n, mask[b], deltas, True)
            want = sr.features(Cs.clean(cep[b]), e, mask[b], deltas, True)
            assert got.dtype == np.float32 and not got[e:].any()
            if e:
                assert np.abs(got - want).max() <= Cs.feat_bound(float(np.abs(cep[b, :e]).max())), (n_coef, deltas, b)
            # integer cepstra: every difference and the fused sum are exact, the float64 column sums are exact in any order,
            # so the order-following restatement and the plain float32 one agree bit for bit
            gi = sr.features_f32(icep[b], n, imask[b], deltas, True)
            wi = sr.features(Cs.clean(icep[b]), e, imask[b], deltas, True, dtype=np.float32)
            assert np.array_equal(gi, wi), (n_coef, deltas, b)
    one = np.zeros(20, np.uint8)
    one[13] = 1
    cep = Cs.feat_batch(n_coef)[0][7, :20]
    f = sr.features_f32(cep, 20, one, True, True)
    assert not f[13].any() and f[12].any()                                       # the one kept frame is the mean


def test_score_cases_are_exact_where_they_say_and_bounded_elsewhere():
    a, b_, mask = Cs.score_batch(True)
    for u, n in enumerate(Cs.SCORE_LENS):
        assert np.isnan(a[u, n:]).all() and (mask[u, n:] != 0).all()
        assert np.array_equal(a[u, :n], np.round(a[u, :n]))
        cnt, sa, sb, sl = sr.score(Cs.clean(a[u]), Cs.clean(b_[u]), n, mask[u])
        if cnt:
            keep = Cs.kept([n], a.shape[1], mask[u:u + 1])[0]
            assert sa * cnt == a[u][keep].astype(np.int64).sum() or abs(sa * cnt - a[u][keep].astype(np.int64).sum()) < 1e-9
    a, b_, mask = Cs.score_batch(False)
    assert (Cs.kept(Cs.SCORE_LENS, a.shape[1], mask).sum(1)[1:] >= 0).all() and Cs.kept(Cs.SCORE_LENS, a.shape[1], mask)[5].sum() > 256


@pytest.mark.parametrize('shape', Cs.PREP_SHAPES)
def test_prepare_bound_holds_the_reference_and_a_zero_weight_gives_minus_infinity(shape):
    S, M, D = shape
    w, mu, var = Cs.prep_model(S, M, D, zero_weight=M // 2)
    c, bound = Cs.c_reference(w, var)
    assert np.isneginf(c[M // 2]) and np.isfinite(np.delete(c, M // 2)).all() and np.isfinite(bound).all()
    with np.errstate(divide='ignore'):
        want = sr.log_norm(w, var)
    live = np.isfinite(c)
    assert (np.abs(want[live].astype(np.float32).astype(np.float64) - c[live]) <= bound[live]).all()
    assert var.min() >= 1e-4 * 0.99 and var.max() <= 50.0 * 1.01
