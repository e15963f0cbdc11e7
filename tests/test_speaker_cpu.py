"""Speaker similarity without a GPU: the numpy reference (tests/speaker_ref.py) on the synthetic speakers -- a
non-decreasing EM trace, every utterance closest to its own speaker's model, the MAP corner cases, the float32 control
inside the per-frame bound --, every ValueError of speaker.py, the new exports and the workspace arithmetic."""
import os
import re

import numpy as np
import pytest

import speaker_ref as sr
from conftest import ROOT

NEW = ('vc_gmm_tile_frames', 'vc_gmm_partitions', 'vc_gmm_table_floats', 'vc_gmm_workspace_bytes', 'vc_spk_features_f32',
       'vc_gmm_prepare_f32', 'vc_gmm_loglik_f32', 'vc_gmm_score_f32', 'vc_gmm_accumulate_f32', 'vc_gmm_update_f32')


@pytest.fixture(scope='module')
def world():
    """The synthetic set, a 16-component UBM of 8 iterations, one MAP model per speaker and the LLR of every utterance
    against every model, all from the float64 reference."""
    x, lens, spk = sr.synthetic_speakers()
    w, mu, var, trace = sr.fit(x, lens, 16, 8)
    st = sr.accumulate(x, lens, spk, 4, w, mu, var)
    means = sr.update_map(st['N'], st['S1'], mu)
    llr = np.zeros((len(lens), 4))
    for b, n in enumerate(lens):
        ubm = sr.loglik(x[b, :n], w, mu, var)[0]
        for s in range(4):
            llr[b, s] = sr.score(sr.loglik(x[b, :n], w, means[s], var)[0], ubm, n)[3]
    return dict(x=x, lens=lens, spk=spk, ubm=(w, mu, var), trace=trace, means=means, llr=llr)


def test_the_em_trace_of_the_reference_never_falls(world):
    t = world['trace']
    print('trace', t)
    assert len(t) == 8 and np.all(np.diff(t) >= 0.0) and t[-1] > t[0] + 0.1


def test_the_reference_separates_the_synthetic_speakers(world):
    llr, spk = world['llr'], world['spk']
    own = llr[np.arange(len(spk)), spk]
    other = np.where(np.arange(4)[None] == spk[:, None], -np.inf, llr).max(1)
    print('smallest own-model LLR %.3f, largest other-model LLR %.3f, smallest margin %.3f' % (own.min(), other.max(), (own - other).min()))
    assert (own > other).all()
    assert own.min() > other.max()                                  # every own-model LLR above every other-model LLR


def test_the_smoke_case_separates_in_the_reference():
    """smoke()'s speaker case on the float64 reference: mean-only MAP of a background model whose components ARE the
    speakers moves nothing (every LLR is then rounding noise), so the case must keep the speakers apart inside the
    components.  Own-model LLRs are positive, other-model LLRs negative, both well away from the 0.1 smoke() asserts."""
    import __graft_entry__ as g
    x, lens, who = g._smoke_speaker_data()
    w, mu, var, trace = sr.fit(x, lens, 2, 4)
    st = sr.accumulate(x, lens, who, 2, w, mu, var)
    means = sr.update_map(st['N'], st['S1'], mu)
    for b, n in enumerate(lens):
        ubm = sr.loglik(x[b, :n], w, mu, var)[0]
        llr = [sr.score(sr.loglik(x[b, :n], w, means[s], var)[0], ubm, n)[3] for s in range(2)]
        assert llr[who[b]] > 0.2 and llr[1 - who[b]] < -0.5, (b, llr)
    assert trace[-1] >= trace[0]


def test_map_corner_cases():
    rng = np.random.RandomState(2)
    G, M, D = 3, 4, 5
    ubm = rng.standard_normal((M, D)).astype(np.float32)
    N = rng.uniform(1.0, 30.0, (G, M))
    N[1] = 0.0                                                      # a group without utterances
    N[2, 3] = 0.0                                                   # a component the speaker never visits
    mean = rng.standard_normal((G, M, D))
    S1 = mean * N[..., None]
    got = sr.update_map(N, S1, ubm, 16.0)
    assert got.dtype == np.float32 and np.array_equal(got[1], ubm) and np.array_equal(got[2, 3], ubm[3])
    a = N[0] / (N[0] + 16.0)
    assert np.allclose(got[0], a[:, None] * mean[0] + (1 - a[:, None]) * ubm, rtol=1e-6, atol=1e-6)
    assert np.allclose(sr.update_map(N[:1], S1[:1], ubm, 0.0)[0], mean[0], rtol=1e-6, atol=1e-6)       # relevance 0: the data's mean
    big = sr.update_map(N[:1] * 1e9, S1[:1] * 1e9, ubm, 16.0)[0]
    assert np.allclose(big, mean[0], rtol=1e-6, atol=1e-6)


def test_em_update_corner_cases():
    M, D = 3, 2
    N = np.array([10.0, 0.5, 0.0])
    S1 = np.array([[10.0, 20.0], [0.5, 0.5], [0.0, 0.0]])
    S2 = np.array([[10.0 + 10 * 4.0, 40.0 + 10 * 1e-6], [1.0, 1.0], [0.0, 0.0]])
    old_mu, old_var = np.full((M, D), 7.0, np.float32), np.full((M, D), 3.0, np.float32)
    w, mu, var = sr.update_em(N, S1, S2, old_mu, old_var, np.array([0.01, 0.01], np.float32), 1.0)
    assert np.array_equal(mu[0], [1.0, 2.0]) and var[0, 0] == np.float32(4.0) and var[0, 1] == np.float32(0.01)     # the floor binds in one dimension
    assert np.array_equal(mu[1:], old_mu[1:]) and np.array_equal(var[1:], old_var[1:])                           # below min_count: kept
    assert w[2] == np.float32(2.0 ** -40) and w[0] == np.float32(10.0 / 10.5)                                     # floored, not renormalised


def test_the_float32_control_stays_inside_the_frame_bound(world):
    """The reference run in float32 against itself in float64 on the synthetic set and on a harder model (a component with
    a variance 10^-4 of the others, a frame 40 standard deviations out): the bound the device is held to must hold for
    plain float32 arithmetic here first."""
    x, lens = world['x'], world['lens']
    w, mu, var = world['ubm']
    worst = 0.0
    for b in (0, 7, 23):
        xb = x[b, :lens[b]]
        l64, E = sr.loglik(xb, w, mu, var)
        l32, _ = sr.loglik(xb, w, mu, var, np.float32)
        worst = max(worst, float((np.abs(l32 - l64) / sr.frame_bound(8, 16, E)).max()))
    for D, M in ((1, 1), (8, 2), (48, 65), (64, 256)):
        xs, ws, ms, vs = hard_case(D, M, 70, seed=D + M)
        l64, E = sr.loglik(xs, ws, ms, vs)
        l32, _ = sr.loglik(xs, ws, ms, vs, np.float32)
        r = float((np.abs(l32 - l64) / sr.frame_bound(D, M, E)).max())
        print('D %2d M %3d: float32 control error / bound = %.3f' % (D, M, r))
        worst = max(worst, r)
    print('largest float32-control error / bound: %.3f' % worst)
    assert worst <= 1.0


def hard_case(D, M, n, seed):
    """n frames around a random M-component model in D dimensions; component 0 has a variance 10^-4 of the others and a
    few frames sit on it; the last frame lies 40 standard deviations from every mean."""
    rng = np.random.RandomState(seed)
    mu = rng.standard_normal((M, D)).astype(np.float32)
    var = (0.5 + rng.rand(M, D)).astype(np.float32)
    var[0] *= np.float32(1e-4)
    w = rng.dirichlet(np.full(M, 3.0)).astype(np.float32)
    k = rng.randint(0, M, n)
    k[:4] = 0
    x = (mu[k] + np.sqrt(var[k]) * rng.standard_normal((n, D))).astype(np.float32)
    x[-1] = (mu.mean(0) + 40.0 * np.sqrt(var.max(0)) * np.sign(rng.standard_normal(D)) + np.abs(mu).max(0)).astype(np.float32)
    return x, w, mu, var


def test_features_reference_properties():
    rng = np.random.RandomState(5)
    c = rng.standard_normal((9, 3)).astype(np.float32)
    f = sr.features(c, 7)
    assert f.shape == (9, 6) and not f[7:].any() and np.allclose(f[:7].mean(0), 0.0, atol=1e-12)
    ramp = np.arange(9, dtype=np.float64)[:, None] * np.array([[1.0, -2.0]])
    d = sr.features(ramp, 9, cmn=False)
    assert np.allclose(d[2:7, 2:], [[1.0, -2.0]])                   # the regression of a ramp is its slope away from the clamps
    one = sr.features(c, 1, cmn=False)
    assert np.array_equal(one[0, :3], c[0].astype(np.float64)) and not one[0, 3:].any()
    none = sr.features(c, 7, mask=np.zeros(9, bool))
    assert np.array_equal(none, sr.features(c, 7, cmn=False))      # no kept frame: nothing subtracted


def test_exports_header_and_binding():
    import _vc
    import speaker
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _vc.lib()
    for name in NEW:
        m = re.search(r'\b%s\s*\(([^;{}]*?)\)\s*;' % name, code)
        assert m and name in _vc._SIGS and hasattr(lib, name), name
        n_c = 0 if m.group(1).strip() in ('', 'void') else len(m.group(1).split(','))
        assert n_c == len(_vc._SIGS[name][1]), name
    assert lib.vc_version() == _vc.VC_ABI_VERSION == 7             # added without a version bump
    assert 'Speaker' in hdr and os.path.exists(os.path.join(ROOT, 'speech-cloner_amd', 'csrc', 'vc_gmm.hip'))
    assert lib.vc_gmm_tile_frames() == speaker.GMM_TILE_FRAMES


def test_workspace_and_table_arithmetic_at_the_limits():
    import _vc
    lib = _vc.lib()
    blk = lambda D: 64 * (1 + 2 * D) + 1
    up = lambda v: (v + 255) // 256 * 256
    assert [lib.vc_gmm_partitions(g) for g in (1, 2, 3, 64, 65, 128, 4096)] == [128, 64, 42, 2, 1, 1, 1]
    assert lib.vc_gmm_partitions(0) == 0 and lib.vc_gmm_partitions(4097) == 0
    assert lib.vc_gmm_workspace_bytes(1, 256, 64) == up(128 * 4 * blk(64) * 8) == 33820672
    assert lib.vc_gmm_workspace_bytes(64, 256, 64) == 33820672 and lib.vc_gmm_workspace_bytes(3, 16, 8) == up(3 * 42 * blk(8) * 8)
    assert lib.vc_gmm_workspace_bytes(65, 256, 64) == 0 and lib.vc_gmm_workspace_bytes(4096, 256, 64) == 0      # P = 1: no workspace
    assert max(lib.vc_gmm_workspace_bytes(g, 256, 64) for g in range(1, 130)) <= 64 * 2 ** 20
    for bad in ((0, 16, 8), (4097, 16, 8), (1, 257, 8), (1, 16, 65), (1, 0, 8), (1, 16, 0)):
        assert lib.vc_gmm_workspace_bytes(*bad) == 0, bad
    assert lib.vc_gmm_table_floats(1, 16, 8) == 2 * 16 * 8 + 16 and lib.vc_gmm_table_floats(4097, 256, 64) == 4098 * 256 * 64 + 256
    assert lib.vc_gmm_table_floats(4098, 256, 64) == 0


def test_the_exports_refuse_bad_arguments_before_any_launch():
    import ctypes
    import _vc
    lib = _vc.lib()
    p = ctypes.c_void_p(4096)                                       # never dereferenced
    assert lib.vc_spk_features_f32(None, p, None, 1, 10, 4, 1, 1, p, None) == 1 and b'vc_spk_features_f32' in lib.vc_last_error()
    assert lib.vc_spk_features_f32(p, p, None, 1, 10, 33, 1, 1, p, None) == 4
    assert lib.vc_spk_features_f32(p, p, None, 1, 2 ** 25, 32, 1, 1, p, None) == 4       # frames * D beyond 2^30
    assert lib.vc_gmm_prepare_f32(p, p, p, 1, 257, 8, p, None) == 4 and lib.vc_gmm_prepare_f32(p, p, p, 0, 16, 8, p, None) == 1
    assert lib.vc_gmm_loglik_f32(p, p, 1, 10, 65, p, 1, 16, p, p, None, None, None) == 4
    assert lib.vc_gmm_loglik_f32(p, p, 65536, 10, 8, p, 1, 16, p, p, None, None, None) == 4
    assert lib.vc_gmm_loglik_f32(p, p, 1, 10, 8, p, 1, 16, p, p, p, None, None) == 1      # a second model without its output
    assert lib.vc_gmm_score_f32(p, None, p, None, 0, 10, p, p, None) == 1
    assert lib.vc_gmm_accumulate_f32(p, p, p, None, p, 1, 10, 8, p, 1, 16, 0, 4097, p, p, p, p, None, 0, None) == 4
    assert lib.vc_gmm_accumulate_f32(p, p, p, None, p, 1, 10, 8, p, 1, 16, 1, 1, p, p, p, p, None, 0, None) == 1       # model >= n_models
    assert lib.vc_gmm_accumulate_f32(p, p, p, None, p, 1, 10, 8, p, 1, 16, 0, 1, p, p, p, p, p, 1000, None) == 3       # VC_ERR_WORKSPACE
    assert b'workspace' in lib.vc_last_error()
    assert lib.vc_gmm_update_f32(2, p, p, p, 1, 16, 8, p, p, p, 1.0, 16.0, p, p, p, None) == 1
    assert lib.vc_gmm_update_f32(0, p, p, p, 2, 16, 8, p, p, p, 1.0, 16.0, p, p, p, None) == 1       # EM takes one group
    assert lib.vc_gmm_update_f32(1, p, p, None, 4097, 16, 8, p, None, None, 0.0, 16.0, None, p, None, None) == 4


def test_every_value_error_of_the_python_layer():
    import speaker as sp
    f32 = np.float32
    feat, lens = np.zeros((3, 20, 8), f32), [20, 5, 1]
    ubm = sp.GMM(np.full(4, 0.25, f32), np.zeros((4, 8), f32), np.ones((4, 8), f32))
    means = np.zeros((2, 4, 8), f32)
    mel = np.zeros((3, 20, 80), f32)
    bad = [
        (lambda: sp.features_batch(mel[0], lens), 'mel'),
        (lambda: sp.features_batch(mel, lens, n_coef=33), 'coefficients'),
        (lambda: sp.features_batch(mel, lens, n_coef=24, first_coef=60), 'n_coef'),
        (lambda: sp.features_batch(mel, [20, 5, 0]), 'lens'),
        (lambda: sp.features_batch(mel, [20, 5, 21]), 'lens'),
        (lambda: sp.features_batch(mel, lens, mask=np.ones((3, 19), np.uint8)), 'mask'),
        (lambda: sp.features_batch(mel, lens, mask=np.ones((3, 20), f32)), 'mask'),
        (lambda: sp.gmm_fit(feat[0], lens), 'feat'),
        (lambda: sp.gmm_fit(feat.astype(np.float64), lens), 'float32'),
        (lambda: sp.gmm_fit(np.zeros((3, 20, 65), f32), lens), 'columns'),
        (lambda: sp.gmm_fit(np.broadcast_to(np.zeros((1, 1, 64), f32), (1, 2 ** 24 + 1, 64)), [5]), '2^30'),
        (lambda: sp.gmm_fit(np.broadcast_to(np.zeros((1, 1, 1), f32), (65536, 1, 1)), [1] * 65536), '65535'),
        (lambda: sp.gmm_fit(feat, lens, n_components=0), 'n_components'),
        (lambda: sp.gmm_fit(feat, lens, n_components=257), 'n_components'),
        (lambda: sp.gmm_fit(feat, lens, n_iter=0), 'n_iter'),
        (lambda: sp.gmm_fit(feat, lens, var_floor=0.0), 'var_floor'),
        (lambda: sp.gmm_fit(feat, lens, min_count=-1.0), 'min_count'),
        (lambda: sp.gmm_fit(feat, [20, 5], 4), 'lens'),
        (lambda: sp.gmm_fit(feat, lens, 4, mask=np.ones((3, 21), bool)), 'mask'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, 1, 2], 2), 'groups'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, -2, 1], 2), 'groups'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, 1], 2), 'groups'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, 1, 1], 0), 'n_groups'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, 1, 1], 4097), 'n_groups'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, 1, 1], 2, relevance=-1.0), 'relevance'),
        (lambda: sp.gmm_adapt_batch(ubm, feat, lens, [0, 1, 1], 2, relevance=float('nan')), 'relevance'),
        (lambda: sp.gmm_adapt_batch((ubm.weights, ubm.means), feat, lens, [0, 1, 1], 2), 'ubm'),
        (lambda: sp.gmm_adapt_batch(ubm._replace(means=np.zeros((4, 9), f32)), feat, lens, [0, 1, 1], 2), 'means'),
        (lambda: sp.gmm_adapt_batch(ubm._replace(variances=np.ones((4, 8))), feat, lens, [0, 1, 1], 2), 'variances'),
        (lambda: sp.gmm_adapt_batch(sp.GMM(np.zeros(257, f32), np.zeros((257, 8), f32), np.ones((257, 8), f32)), feat, lens, [0, 1, 1], 2), 'weights'),
        (lambda: sp.gmm_score_batch(ubm, means, feat, lens, [0, 1, 2]), 'model_index'),
        (lambda: sp.gmm_score_batch(ubm, means, feat, lens, [0, -1, 1]), 'model_index'),
        (lambda: sp.gmm_score_batch(ubm, means, feat, lens, [0.0, 1.0, 1.0]), 'model_index'),
        (lambda: sp.gmm_score_batch(ubm, means[0], feat, lens, [0, 0, 0]), 'spk_means'),
        (lambda: sp.gmm_score_batch(ubm, np.zeros((2, 5, 8), f32), feat, lens, [0, 0, 0]), 'spk_means'),
        (lambda: sp.gmm_score_batch(ubm, means.astype(np.float64), feat, lens, [0, 0, 0]), 'spk_means'),
        (lambda: sp.gmm_score_batch(ubm, means, feat, lens, [0, 0, 0], mask=np.ones((2, 20), np.uint8)), 'mask'),
        (lambda: sp.gmm_score_batch(ubm, means, feat, [20, 5, 30], [0, 0, 0]), 'lens'),
    ]
    for call, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            call()


def test_speaker_wav_batch_checks_on_the_host():
    import json
    import speaker as sp
    f32 = np.float32
    c = json.load(open(os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'ds_dec_cfg_d.json')))
    c['hop_length'] = int(c['hop_length_ms'] * c['sample_rate'] / 1000.0)           # test.py:469-470
    c['win_length'] = int(c['win_length_ms'] * c['sample_rate'] / 1000.0)
    ubm = sp.GMM(np.full(4, 0.25, f32), np.zeros((4, 48), f32), np.ones((4, 48), f32))
    means = np.zeros((2, 4, 48), f32)
    wav = np.zeros((2, 4000), f32)
    F = 1 + 4000 // c['hop_length']
    bad = [
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], None), 'cfg_d'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav[0], None, [0, 1], c), 'wav'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, [4000, 4001], [0, 1], c), 'lens'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 2], c), 'model_index'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], c, deltas=False), 'means'),          # D = 24 against a 48-column model
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], c, mask='loud'), 'mode'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], c, mask='energy', top_db=-3.0), 'top_db'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], c, mask='voiced', fmin=1.0), 'fmin'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], c, mask=np.ones((2, F + 1), np.uint8)), 'mask'),
        (lambda: sp.speaker_wav_batch(ubm, means, wav, None, [0, 1], c, res_type='nearest'), 'res_type'),
    ]
    for call, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            call()
