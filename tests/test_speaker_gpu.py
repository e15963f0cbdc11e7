"""Speaker similarity on the device (csrc/vc_gmm.hip, speaker.py) against tests/speaker_ref.py in float64: every kernel alone
at the shapes where it can go wrong, the bit-identities (alone / batched / twice / graph replay), the fit's trace, the
whole chain on the synthetic speakers, speaker_wav_batch against a chain made by hand, and no host synchronisation.

Observed error / bound ratios are printed by every test (pytest -s); the figures of one run are in
profiles/speaker/README.md."""
import numpy as np
import pytest
import torch

import speaker_ref as sr
from test_speaker_cpu import hard_case
from test_convert_batch_gpu import _ragged, f32_models        # noqa: F401  (a fixture and its inputs; that file is not edited)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DS = (1, 8, 48, 64)
MS = (1, 2, 63, 64, 65, 256)


def _np(t):
    return t.cpu().numpy()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype=dtype)


def _i32(a):
    return _dev(np.asarray(a, np.int32))


def _same(a, b):
    """Bit-identical, NaN equal to NaN."""
    if a.dtype.is_floating_point:
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    return torch.equal(a, b)


def _graph(fn):
    """fn() once eagerly, then captured on a side stream; returns (graph, the captured outputs)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = fn()
    return g, out


# ---------------------------------------------------------------------------------------------------------------- features
@pytest.mark.parametrize('cmn', [False, True])
@pytest.mark.parametrize('deltas', [False, True])
@pytest.mark.parametrize('n_coef', [1, 24, 32])
def test_features_against_float64(n_coef, deltas, cmn):
    """Bound, with u = 2^-24 and A the largest |cepstrum| of the utterance.  The delta: two rounded differences of at most
    2 A (2 A u each), their weighted sum of at most 6 A (6 A u), all divided by 10, and the rounded quotient of at most
    0.6 A (0.6 A u): (2 + 4 + 6) / 10 + 0.6 = 1.8 A u.  The mean of n terms is accumulated in float64 (n 2^-53, nothing) from
    features that carry that 1.8 A u, and rounded once (A u); the subtraction of two values of at most A rounds once more
    (2 A u): 1.8 + 1.8 + 1 + 2 = 6.6, taken as 8 A u."""
    import speaker as sp
    rng = np.random.RandomState(100 * n_coef + 10 * deltas + cmn)
    lens = [1, 2, 3, 257, 40, 64]
    B, F = len(lens), 260
    cep = (3.0 * rng.standard_normal((B, F, n_coef))).astype(np.float32)
    mask = (rng.rand(B, F) < 0.7).astype(np.uint8)
    mask[4] = 0                                                     # no frame kept: nothing is subtracted
    mask[0] = 1
    got = _np(sp._features_launch(_dev(cep), _i32(lens), _dev(mask), deltas, cmn))
    assert got.shape == (B, F, n_coef * (2 if deltas else 1))
    worst = 0.0
    for b, n in enumerate(lens):
        want = sr.features(cep[b], n, mask[b], deltas, cmn)
        A = float(np.abs(cep[b, :n]).max())
        worst = max(worst, float(np.abs(got[b] - want).max()) / (8 * U * A))
        assert not got[b, n:].any()
    print('features n_coef %d deltas %d cmn %d: largest error / bound %.3f' % (n_coef, deltas, cmn, worst))
    assert worst <= 1.0
    plain = _np(sp._features_launch(_dev(cep), _i32(lens), _dev(mask), deltas, False))
    assert np.array_equal(got[4], plain[4])                         # the utterance without a kept frame
    if cmn:
        every = _np(sp._features_launch(_dev(cep), _i32(lens), None, deltas, True))
        ones = _np(sp._features_launch(_dev(cep), _i32(lens), _dev(np.ones_like(mask)), deltas, True))
        assert np.array_equal(every, ones)                          # no mask = every frame
        assert np.abs(every[3, :257].astype(np.float64).mean(0)).max() <= 8 * U * float(np.abs(cep[3, :257]).max())      # the mean is gone


def test_features_batch_is_mel_cepstra_then_the_launch():
    import evaluation as ev
    import speaker as sp
    rng = np.random.RandomState(1)
    mel = rng.rand(3, 50, 80).astype(np.float32)
    lens = [50, 17, 1]
    got = sp.features_batch(mel, lens)
    want = sp._features_launch(ev.mel_cepstra(mel), _i32(lens), None, True, True)
    assert got.shape == (3, 50, 48) and torch.equal(got, want)
    one = sp.features_batch(mel[1:2, :17].copy(), [17])
    assert torch.equal(one[0], got[1, :17])                         # alone and in a batch


# ------------------------------------------------------------------------------------------------------------------ loglik
def _case(D, M, seed=0):
    """Six utterances around hard_case's model: 1, tile - 1, tile, tile + 1 frames, 70 frames with the frames that sit on the
    narrow component and the frame 40 standard deviations out, and 50 frames; a second set of means."""
    import speaker as sp
    T = sp.GMM_TILE_FRAMES
    lens = [1, T - 1, T, T + 1, 70, 50]
    x70, w, mu, var = hard_case(D, M, 70, seed=1000 * D + M + seed)
    rng = np.random.RandomState(D * 7 + M)
    F = 72
    x = np.zeros((len(lens), F, D), np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = x70[:n] if b == 4 else x70[rng.randint(0, 69, n)]
        x[b, n:] = 99.0                                             # beyond the length: never read
    mu2 = (mu + 0.2 * rng.standard_normal(mu.shape)).astype(np.float32)
    return dict(x=x, lens=lens, w=w, mu=np.stack([mu, mu2]), var=var, F=F)


def _device_ll(c, model_a, model_b):
    import speaker as sp
    S, M, D = c['mu'].shape
    tab = sp._prepare_launch(_dev(c['w']), _dev(c['mu']), _dev(c['var']))
    return tab, sp._loglik_launch(_dev(c['x']), _i32(c['lens']), tab, S, M, _i32(model_a), None if model_b is None else _i32(model_b))


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('D', DS)
def test_loglik_against_float64(D, M):
    c = _case(D, M)
    ma, mb = [0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0]
    _, (ll_a, ll_b) = _device_ll(c, ma, mb)
    _, (only_a, none) = _device_ll(c, ma, None)
    assert none is None and torch.equal(only_a, ll_a)
    worst = 0.0
    for got, idx in ((_np(ll_a), ma), (_np(ll_b), mb)):
        for b, n in enumerate(c['lens']):
            want, E = sr.loglik(c['x'][b, :n], c['w'], c['mu'][idx[b]], c['var'])
            worst = max(worst, float((np.abs(got[b, :n] - want) / sr.frame_bound(D, M, E)).max()))
            assert not got[b, n:].any()
            assert np.isfinite(got[b, :n]).all()
    print('loglik D %2d M %3d: largest error / bound %.3f' % (D, M, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------- score
@pytest.fixture(scope='module')
def scored():
    import speaker as sp
    c = _case(8, 65)
    rng = np.random.RandomState(3)
    mask = (rng.rand(6, c['F']) < 0.6).astype(np.uint8)
    mask[5] = 0                                                     # no kept frame
    ma = [0, 1, 0, 1, 0, 1]
    _, (ll_a, ll_b) = _device_ll(c, ma, [0] * 6)
    return c, mask, ma, ll_a, ll_b


def test_score_against_float64(scored):
    import speaker as sp
    c, mask, ma, ll_a, ll_b = scored
    r = sp._score_launch(ll_a, ll_b, _i32(c['lens']), _dev(mask))
    n, llr, a, b_ = _np(r.n_frames), _np(r.llr), _np(r.ll_spk), _np(r.ll_ubm)
    worst = 0.0
    for u, L in enumerate(c['lens']):
        keep = mask[u, :L].astype(bool)
        assert n[u] == keep.sum()
        if not keep.any():
            assert np.isnan(llr[u]) and np.isnan(a[u]) and np.isnan(b_[u])
            continue
        wa, Ea = sr.loglik(c['x'][u, :L], c['w'], c['mu'][ma[u]], c['var'])
        wb, Eb = sr.loglik(c['x'][u, :L], c['w'], c['mu'][0], c['var'])
        _, sa, sb, sl = sr.score(wa, wb, L, mask[u, :L])
        ba, bb = sr.frame_bound(8, 65, Ea)[keep].mean(), sr.frame_bound(8, 65, Eb)[keep].mean()
        worst = max(worst, abs(a[u] - sa) / (ba + U * abs(sa)), abs(b_[u] - sb) / (bb + U * abs(sb)), abs(llr[u] - sl) / (ba + bb + U * abs(sl)))
    print('score: largest error / bound %.3f' % worst)
    assert worst <= 1.0 and n[5] == 0
    nomask = sp._score_launch(ll_a, None, _i32(c['lens']), None)
    assert _np(nomask.n_frames).tolist() == c['lens'] and torch.isnan(nomask.llr).all() and torch.isnan(nomask.ll_ubm).all()


def test_score_alone_in_a_batch_twice_and_under_graph_replay(scored):
    import speaker as sp
    c, mask, ma, _, _ = scored
    ubm = sp.GMM(c['w'], c['mu'][0], c['var'])
    full = sp.gmm_score_batch(ubm, c['mu'], c['x'], c['lens'], ma, mask)
    again = sp.gmm_score_batch(ubm, c['mu'], c['x'], c['lens'], ma, mask)
    for k in full._fields:
        assert _same(getattr(full, k), getattr(again, k)), k
    for u in (0, 3, 4, 5):
        n = c['lens'][u]
        one = sp.gmm_score_batch(ubm, c['mu'][ma[u]:ma[u] + 1], c['x'][u:u + 1, :n].copy(), [n], [0], mask[u:u + 1, :n].copy())
        for k in full._fields:
            assert _same(getattr(one, k)[0], getattr(full, k)[u]), (u, k)
    # graph replay on static buffers, then with other contents and lengths
    x, d_len, d_mask = _dev(c['x']), _i32(c['lens']), _dev(mask)
    d_model = _i32(np.asarray(ma) + 1)
    dub, d_means = sp._gmm_to_device(ubm), _dev(c['mu'])
    g, out = _graph(lambda: sp._score_chain(dub, d_means, x, d_len, d_model, d_mask))
    g.replay()
    torch.cuda.synchronize()
    for k in full._fields:
        assert _same(getattr(out, k), getattr(full, k)), k
    c2 = _case(8, 65, seed=5)
    lens2 = [70, 1, 33, 2, 31, 64]
    x.copy_(_dev(c2['x']))
    d_len.copy_(_i32(lens2))
    g.replay()
    torch.cuda.synchronize()
    want = sp.gmm_score_batch(ubm, c['mu'], c2['x'], lens2, ma, mask)
    for k in full._fields:
        assert _same(getattr(out, k), getattr(want, k)), k


# -------------------------------------------------------------------------------------------------------------- accumulate
def _accumulate(c, groups, G, mask, ws=None):
    import speaker as sp
    S, M, D = c['mu'].shape
    tab, (ll, _) = _device_ll(c, [0] * 6, None)
    st = sp._accumulate_launch(_dev(c['x']), ll, _i32(c['lens']), None if mask is None else _dev(mask), _i32(groups), tab, S, M, G, ws=ws)
    return st, ll, tab


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('D', DS)
def test_accumulate_against_float64(D, M):
    """delta = the largest per-frame bound of the frames that count.  gamma = exp(l_m - ll) carries the error of l_m and of
    ll, at most delta each, so every sum of gamma-weighted non-negative terms is off by at most 2 delta of itself: N by
    2 delta N, S1 by 2 delta sum gamma |x|, S2 by 2 delta S2.  The right-hand sides come from the float64 reference."""
    c = _case(D, M)
    rng = np.random.RandomState(D + M)
    mask = (rng.rand(6, c['F']) < 0.8).astype(np.uint8)
    worst = 0.0
    for G, groups, mk in ((1, [0] * 6, None), (3, [0, 2, 0, -1, 2, 0], mask), (1, [0, 0, -1, 0, 0, 0], mask)):
        st, _, _ = _accumulate(c, groups, G, mk)
        want = sr.accumulate(c['x'], c['lens'], groups, G, c['w'], c['mu'][0], c['var'], mk)
        delta = 0.0
        for b, n in enumerate(c['lens']):
            if 0 <= groups[b] < G:
                delta = max(delta, float(sr.frame_bound(D, M, sr.loglik(c['x'][b, :n], c['w'], c['mu'][0], c['var'])[1]).max()))
        tiny = 1e-300
        rN = np.abs(_np(st.N) - want['N']) / (2 * delta * want['N'] + tiny)
        r1 = np.abs(_np(st.S1) - want['S1']) / (2 * delta * want['A1'] + tiny)
        r2 = np.abs(_np(st.S2) - want['S2']) / (2 * delta * want['S2'] + tiny)
        rL = np.abs(_np(st.L) - want['L']) / (delta * np.maximum(want['N'].sum(1), 1.0))
        worst = max(worst, float(rN.max()), float(r1.max()), float(r2.max()), float(rL.max()))
        if G == 3:
            assert not _np(st.N)[1].any() and not _np(st.S1)[1].any() and not _np(st.S2)[1].any() and _np(st.L)[1] == 0.0     # the empty group
        kept = sum(int((np.ones(n) if mk is None else mk[b, :n]).sum()) for b, n in enumerate(c['lens']) if 0 <= groups[b] < G)
        assert abs(float(_np(st.N).sum()) - kept) <= 1e-4 * max(kept, 1)               # responsibilities sum to one per frame
    print('accumulate D %2d M %3d: largest error / bound %.3f' % (D, M, worst))
    assert worst <= 1.0


def test_accumulate_twice_under_graph_replay_and_its_workspace():
    import _vc
    import speaker as sp
    c = _case(48, 65)
    groups = [0, 2, 0, -1, 2, 0]
    rng = np.random.RandomState(9)
    mask = (rng.rand(6, c['F']) < 0.8).astype(np.uint8)
    for G, gr in ((1, [0] * 6), (3, groups), (70, [69, 2, 0, -1, 2, 69])):         # 70 groups: one partition, no workspace
        a, ll, tab = _accumulate(c, gr, G, mask)
        b_, _, _ = _accumulate(c, gr, G, mask)
        for k in a._fields:
            assert torch.equal(getattr(a, k), getattr(b_, k)), (G, k)
        need = sp.workspace_bytes(G, 65, 48)
        P = _vc.lib().vc_gmm_partitions(G)
        assert need == (0 if P == 1 else (G * P * 2 * (64 * 97 + 1) * 8 + 255) // 256 * 256)
        x, d_len, d_mask, d_g = _dev(c['x']), _i32(c['lens']), _dev(mask), _i32(gr)
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device='cuda')
        g, out = _graph(lambda: sp._accumulate_launch(x, ll, d_len, d_mask, d_g, tab, 2, 65, G, ws=ws))
        ws.fill_(255)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        for k in a._fields:
            assert torch.equal(getattr(out, k), getattr(a, k)), (G, k)
        if G == 3:
            want = sr.accumulate(c['x'], c['lens'], gr, G, c['w'], c['mu'][0], c['var'], mask)
            assert np.allclose(_np(a.N), want['N'], rtol=1e-4, atol=1e-9)
    small = torch.empty((sp.workspace_bytes(1, 65, 48) - 256,), dtype=torch.uint8, device='cuda')
    with pytest.raises(_vc.VCError, match='workspace'):
        _accumulate(c, [0] * 6, 1, None, ws=small)


# ------------------------------------------------------------------------------------------------------------------ update
def _ulps(got, want):
    want = want.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def test_update_em_and_map_against_the_reference():
    import speaker as sp
    rng = np.random.RandomState(4)
    M, D, G = 65, 48, 3
    N = rng.uniform(2.0, 50.0, (G, M))
    mean = rng.standard_normal((G, M, D))
    v = rng.uniform(0.2, 2.0, (G, M, D))
    N[0, 3] = 0.0                                                   # zero occupancy
    N[0, 4] = 0.5                                                   # below min_count
    N[1] = 0.0                                                      # the empty group
    N[2, 7] = 0.0
    v[0, 5, 2] = 1e-5                                               # the floor binds in one dimension only
    S1, S2 = mean * N[..., None], (v + mean * mean) * N[..., None]
    mu_old = rng.standard_normal((M, D)).astype(np.float32)
    var_old = rng.uniform(0.5, 1.5, (M, D)).astype(np.float32)
    floor = np.full(D, 0.01, np.float32)
    st = sp._STATS(_dev(N[:1]), _dev(S1[:1]), _dev(S2[:1]), _dev(np.zeros(1)))
    w, mu, var = (_np(t) for t in sp._update_em_launch(st, _dev(mu_old), _dev(var_old), _dev(floor), 1.0))
    ww, wm, wv = sr.update_em(N[0], S1[0], S2[0], mu_old, var_old, floor, 1.0)
    worst = max(_ulps(w, ww).max(), _ulps(mu, wm).max(), _ulps(var, wv).max())
    assert np.array_equal(mu[3:5], mu_old[3:5]) and np.array_equal(var[3:5], var_old[3:5])
    assert w[3] == np.float32(2.0 ** -40) and var[5, 2] == np.float32(0.01) and (var[5, :2] > 0.1).all() and (var[5, 3:] > 0.1).all()
    stg = sp._STATS(_dev(N), _dev(S1), _dev(S2), _dev(np.zeros(G)))
    got = _np(sp._update_map_launch(stg, _dev(mu_old), 16.0))
    want = sr.update_map(N, S1, mu_old, 16.0)
    worst = max(worst, _ulps(got, want).max())
    print('update: largest difference %.2f ulp' % worst)
    assert worst <= 2.0
    assert np.array_equal(got[1], mu_old) and np.array_equal(got[2, 7], mu_old[7]) and np.array_equal(got[0, 3], mu_old[3])


# --------------------------------------------------------------------------------------------------------------------- fit
@pytest.fixture(scope='module')
def world():
    """The synthetic speakers, the device's UBM (16 components, 8 iterations), its trace, the adapted means and the scores
    of every utterance against every model -- computed once, shared by the tests below."""
    import speaker as sp
    x, lens, spk = sr.synthetic_speakers()
    dx = _dev(x)
    ubm, trace = sp.gmm_fit(dx, lens, 16, 8)
    means = sp.gmm_adapt_batch(ubm, dx, lens, spk, 4)
    B = len(lens)
    llr = np.stack([_np(sp.gmm_score_batch(ubm, means, dx, lens, [s] * B).llr) for s in range(4)], 1)
    return dict(x=x, dx=dx, lens=lens, spk=spk, ubm=ubm, trace=_np(trace), means=means, llr=llr)


def test_fit_trace_against_the_reference(world):
    """Tolerance: three times the largest gap between the reference's own float32 and float64 traces, and not less than the
    one-step bound delta (the largest per-frame bound under the final model); printed, recorded in
    profiles/speaker/README.md."""
    x, lens = world['x'], world['lens']
    w64, mu64, var64, t64 = sr.fit(x, lens, 16, 8)
    _, _, _, t32 = sr.fit(x, lens, 16, 8, dtype=np.float32)
    gap = float(np.abs(t32 - t64).max())
    delta = max(float(sr.frame_bound(8, 16, sr.loglik(x[b, :n], w64, mu64, var64)[1]).max()) for b, n in enumerate(lens))
    tol = max(3.0 * gap, delta)
    got = world['trace']
    err = float(np.abs(got - t64).max())
    print('fit: reference float32 against float64 %.3e, one-step bound %.3e, tolerance %.3e, device against float64 %.3e' % (gap, delta, tol, err))
    print('fit: device trace', got)
    assert got.shape == (8,) and got.dtype == np.float64
    assert err <= tol
    assert (np.diff(got) >= -tol).all() and got[-1] > got[0] + 0.1
    wd = _np(world['ubm'].weights)
    assert abs(float(wd.sum()) - 1.0) < 1e-5 and (_np(world['ubm'].variances) > 0).all()


def test_end_to_end_separates_the_speakers_as_the_reference_does(world):
    llr, spk, lens, x = world['llr'], world['spk'], world['lens'], world['x']
    own = llr[np.arange(len(spk)), spk]
    other = np.where(np.arange(4)[None] == spk[:, None], -np.inf, llr)
    print('device: smallest own-model LLR %.4f, largest other-model LLR %.4f' % (own.min(), other.max()))
    assert own.min() > other.max()
    w, mu, var = (_np(t) for t in world['ubm'])
    means = _np(world['means'])
    worst = 0.0
    for b, n in enumerate(lens):
        ub, Eu = sr.loglik(x[b, :n], w, mu, var)
        for s in range(4):
            sp_, Es = sr.loglik(x[b, :n], w, means[s], var)
            want = sr.score(sp_, ub, n)[3]
            bound = sr.frame_bound(8, 16, Es).mean() + sr.frame_bound(8, 16, Eu).mean() + U * abs(want)
            worst = max(worst, abs(llr[b, s] - want) / bound)
    print('end to end: largest LLR error / bound %.3f' % worst)
    assert worst <= 1.0
    # the adapted means against the reference's MAP on the device's own UBM
    st = sr.accumulate(x, lens, spk, 4, w, mu, var)
    assert np.allclose(means, sr.update_map(st['N'], st['S1'], mu), rtol=0, atol=1e-4)


# --------------------------------------------------------------------------------------------------------------- waveforms
@pytest.fixture(scope='module')
def wav_world(f32_models):
    """The ragged batch's features and a small UBM with two speaker models fitted on them (D = 48)."""
    import audio_lib
    import speaker as sp
    from test_conversion_gpu import _fe_kwargs
    c = f32_models[4]
    wav, lens = _ragged()
    mel = audio_lib.calc_MFCC_input_batch(torch.from_numpy(wav).cuda(), lens, **_fe_kwargs(c))[1]
    frames = [1 + n // c['hop_length'] for n in lens]
    feat = sp.features_batch(mel, frames)
    ubm, _ = sp.gmm_fit(feat, frames, 8, 2)
    means = sp.gmm_adapt_batch(ubm, feat, frames, [0, 1, 0], 2)
    torch.cuda.synchronize()
    return dict(c=c, wav=wav, lens=lens, ubm=ubm, means=means, kw=_fe_kwargs(c))


def test_speaker_wav_batch_is_the_chain_made_by_hand(wav_world):
    import audio_lib
    import evaluation as ev
    import speaker as sp
    w = wav_world
    c, ubm, means, idx = w['c'], w['ubm'], w['means'], [1, 0, 1]
    hop = c['hop_length']
    # at the configuration's own rate
    got = sp.speaker_wav_batch(ubm, means, w['wav'], w['lens'], idx, c)
    mel = audio_lib.calc_MFCC_input_batch(torch.from_numpy(w['wav']).cuda(), w['lens'], **w['kw'])[1]
    frames = [1 + n // hop for n in w['lens']]
    feat = sp.features_batch(mel, frames)
    want = sp.gmm_score_batch(ubm, means, feat, frames, idx)
    assert torch.equal(got.feat, feat) and got.mask is None
    for k in want._fields:
        assert _same(getattr(got, k), getattr(want, k)), k
    assert _np(got.n_frames).tolist() == frames and torch.isfinite(got.llr).all()
    # from another rate
    sr_in = 22050
    lens_in = [int(n * sr_in / 16000) for n in w['lens']]
    wav_in = np.zeros((3, max(lens_in)), np.float32)
    rng = np.random.RandomState(2)
    for b, n in enumerate(lens_in):
        wav_in[b, :n] = 0.1 * rng.standard_normal(n)
    got = sp.speaker_wav_batch(ubm, means, wav_in, lens_in, idx, c, wav_sr=sr_in)
    x, lens16 = audio_lib.resample_batch(wav_in, lens_in, sr_in, c['sample_rate'])
    mel = audio_lib.calc_MFCC_input_batch(x, lens16, **w['kw'])[1]
    frames = [1 + int(n) // hop for n in lens16]
    feat = sp.features_batch(mel, frames)
    want = sp.gmm_score_batch(ubm, means, feat, frames, idx)
    assert torch.equal(got.feat, feat)
    for k in want._fields:
        assert _same(getattr(got, k), getattr(want, k)), k
    # mask='energy': the mask of activity_batch, the mel with the gain over the speech samples, the mask in the mean and the score
    got = sp.speaker_wav_batch(ubm, means, w['wav'], w['lens'], idx, c, mask='energy')
    act = ev.activity_batch(w['wav'], w['lens'], hop_length=hop, frame_length=c['win_length'])
    frames = [1 + n // hop for n in w['lens']]
    xd, d_len = torch.from_numpy(w['wav']).cuda(), _i32(w['lens'])
    mel = ev._speech_mel(xd, d_len, act.mask, act.n_active, c)
    feat = sp.features_batch(mel, frames, mask=act.mask)
    want = sp.gmm_score_batch(ubm, means, feat, frames, idx, mask=act.mask)
    assert torch.equal(got.mask, act.mask) and torch.equal(got.feat, feat)
    for k in want._fields:
        assert _same(getattr(got, k), getattr(want, k)), k
    assert (_np(got.n_frames) == _np(act.n_active)).all()
    given = sp.speaker_wav_batch(ubm, means, w['wav'], w['lens'], idx, c, mask=_np(act.mask))         # a [B, F] array is taken as given
    assert torch.equal(given.n_frames, got.n_frames)


def test_no_host_synchronisation_inside_fit_and_speaker_wav_batch(world, wav_world):
    import speaker as sp
    w = wav_world
    xd = torch.from_numpy(w['wav']).cuda()
    calls = (lambda: sp.gmm_fit(world['dx'], world['lens'], 16, 3),
             lambda: sp.gmm_adapt_batch(world['ubm'], world['dx'], world['lens'], world['spk'], 4),
             lambda: sp.speaker_wav_batch(w['ubm'], w['means'], xd, w['lens'], [1, 0, 1], w['c']),
             lambda: sp.speaker_wav_batch(w['ubm'], w['means'], xd, w['lens'], [1, 0, 1], w['c'], mask='energy'))
    first = [c() for c in calls]
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.equal(outs[0][1], first[0][1]) and torch.equal(outs[0][0].means, first[0][0].means)
    assert torch.equal(outs[1], first[1]) and _same(outs[2].llr, first[2].llr) and _same(outs[3].llr, first[3].llr)
    assert torch.equal(outs[0][1][:3], torch.from_numpy(world['trace'][:3]).cuda())        # three iterations are the first three of eight
