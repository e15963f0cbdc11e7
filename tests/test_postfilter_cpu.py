"""The postfilters' definition on the CPU (tests/postfilter_ref.py), the host side of speech-cloner_amd/postfilter.py, the
host validation of the four entry points, the compiler's resource report of their kernels and the over-smoothing
experiment of DESIGN.md section 28.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import postfilter_ref as pr

HI = 20.0 * np.log(10.0) / 20.0


def _traj(seed, B, F, C, dtype=np.float32):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, F + 1, C))
    return (0.45 + 0.08 * (0.7 * z[:, 1:] + 0.7 * z[:, :-1])).astype(dtype)


def _coef(seed, C, scale=0.2):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((C, pr.M, 2)) * [1.0, 2.0]).astype(np.float32)


@pytest.mark.parametrize('F', [1, 31, 32, 33, 64, 65, 97])
def test_half_overlapped_windows_sum_to_one(F):
    """Every frame of an utterance lies in two segments, at t and at t + 32; the float32 window's two weights there sum to 1
    within 4 ulp, so a gain that is the same in every bin scales the deviation from the mean by exactly that gain."""
    w = pr.window(np.float32).astype(np.float64)
    assert w[0] == 0.0 and w[32] == 1.0 and np.array_equal(w[1:], w[:0:-1])
    tot = np.zeros(F)
    pos = pr.H * np.arange((F + pr.H - 1) // pr.H + 1)[:, None] - pr.H + np.arange(pr.L)[None, :]
    np.add.at(tot, pos[(pos >= 0) & (pos < F)], np.broadcast_to(w, pos.shape)[(pos >= 0) & (pos < F)])
    assert np.abs(tot - 1.0).max() <= 4 * 2.0 ** -24
    assert pr.segment_index(F).shape == ((F + 31) // 32 + 1, 64) and pr.segment_index(F).min() == 0 and pr.segment_index(F).max() == F - 1


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_zero_coefficients_and_alpha_zero_return_the_input(dtype):
    x = _traj(1, 3, 97, 5)
    x[0, 3, 2] = -0.0
    n = [97, 40, 0]
    st = pr.traj_stats(x, n, np.float32)
    y = pr.ms_filter(x, n, st, np.zeros((5, pr.M, 2), np.float32), -HI, HI, dtype)
    z = pr.gv_filter(x, n, st, np.full(5, 0.02, np.float32), 0.0, 4.0, dtype)
    for out in (y, z):
        assert out.dtype == dtype
        for b, k in enumerate(n):
            assert np.array_equal(out[b, :k].astype(np.float32).view(np.uint32), x[b, :k].view(np.uint32)) and not out[b, k:].any()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_one_frame_and_constant_channels_return_the_input(dtype):
    """The mean is taken about the first frame, so a constant channel's mean is its value and every deviation an exact 0:
    nothing is above the floor, the variance is 0, and both filters pass the channel through whatever the tables say."""
    x = _traj(2, 2, 70, 4)
    x[:, :, 1] = np.float32(0.3)                                     # 0.3 is not a sum-friendly value: n * 0.3 rounds
    n = [70, 1]
    st = pr.traj_stats(x, n, dtype)
    assert np.array_equal(st[:, 1, 0], np.full(2, np.float32(0.3), dtype)) and not st[:, 1, 1].any() and not st[1, :, 1].any()
    st = st.astype(np.float32)
    y = pr.ms_filter(x, n, st, _coef(3, 4), -HI, HI, dtype)
    z = pr.gv_filter(x, n, st, np.full(4, 0.5, np.float32), 1.0, 4.0, dtype)
    ms = pr.ms_stats(x, n, st, dtype)
    assert not ms[0, 1].any() and not ms[1].any() and ms[0, 0, :, 0].min() >= 1
    for out in (y, z):
        assert np.array_equal(out[0, :, 1], x[0, :, 1].astype(dtype)) and np.array_equal(out[1, :1], x[1, :1].astype(dtype))
        assert np.abs(out[0, :, 0] - x[0, :, 0]).max() > 1e-3           # ... while a channel that moves is changed


def test_correction_is_linear_in_the_gain_minus_one():
    x = _traj(4, 1, 130, 3).astype(np.float64)
    st = pr.traj_stats(x)
    h = np.random.default_rng(5).uniform(-0.3, 0.3, (3, pr.M))
    table = lambda t: np.stack([np.zeros_like(h), np.log1p(t * h)], -1)
    y1, y2 = (pr.ms_filter(x, None, st, table(t), -50.0, 50.0) for t in (1.0, 2.0))
    assert np.abs(y1 - x).max() > 1e-3
    assert np.abs((y2 - x) - 2.0 * (y1 - x)).max() <= 1e-13
    # the same gain in every bin but 0 scales the deviation left after the segment's own mean is gone; with bin 0 too it
    # would scale x - mean itself: the windows sum to 1
    g = pr.ms_filter(x, None, st, table(1.0) * 0 + [0.0, np.log(1.5)], -50.0, 50.0)
    v, re, im = pr.spectra(x[0], st[0, :, 0])
    dc = (re[:, 0] / 64.0)                                            # every segment's mean of v
    want = x[0] + 0.5 * ((x[0] - st[0, :, 0]) - (dc[:-1, None] + dc[1:, None]).repeat(32, 1).reshape(-1, 3)[:130])
    assert np.abs(g[0] - want).max() <= 1e-8                            # (the float32 window sums to 1 within 4 ulp)


def test_parseval_between_a_segment_and_its_33_bins():
    x = _traj(6, 1, 97, 2).astype(np.float64)
    v, re, im = pr.spectra(x[0], x[0].mean(0))
    p = re * re + im * im
    wgt = np.where((np.arange(pr.M) == 0) | (np.arange(pr.M) == 32), 1.0, 2.0)[None, :, None]
    assert np.abs((v * v).sum(1) - (wgt * p).sum(1) / 64.0).max() <= 1e-14
    X = np.fft.rfft(v, axis=1)
    assert np.abs(X.real - re).max() <= 1e-13 and np.abs(X.imag - im).max() <= 1e-13


def test_gv_lands_on_the_target_variance():
    x = _traj(7, 1, 400, 6).astype(np.float64)
    gv_t = np.linspace(0.001, 0.03, 6)
    st = pr.traj_stats(x)
    y = pr.gv_filter(x, None, st, gv_t, 1.0, 1e6)
    got = pr.traj_stats(y)
    assert np.abs(got[0, :, 1] / gv_t - 1.0).max() <= 1e-12 and np.abs(got[0, :, 0] - st[0, :, 0]).max() <= 1e-15
    half = pr.traj_stats(pr.gv_filter(x, None, st, gv_t, 0.5, 1e6))
    want = (1.0 + 0.5 * (np.sqrt(gv_t / st[0, :, 1]) - 1.0)) ** 2 * st[0, :, 1]
    assert np.abs(half[0, :, 1] / want - 1.0).max() <= 1e-12
    # the clamp: a target 100 times the variance asks for g = 10, g_max = 4 gives 16 times the variance
    y = pr.gv_filter(x, None, st, 100.0 * st[0, :, 1], 1.0, 4.0)
    assert np.abs(pr.traj_stats(y)[0, :, 1] / (16.0 * st[0, :, 1]) - 1.0).max() <= 1e-12
    # g = 1 where the target is not positive or the variance not above 2^-40
    st2 = st.copy()
    st2[0, 0, 1] = 2.0 ** -40
    y = pr.gv_filter(x, None, st2, np.array([0.01, 0.0, -1.0, np.nan, 0.01, 0.01]), 1.0, 4.0)
    assert np.array_equal(y[0, :, :4], x[0, :, :4]) and np.abs(y[0, :, 4:] - x[0, :, 4:]).max() > 1e-3


def _model(C=3):
    import postfilter
    mu_N, mu_G = np.full((C, pr.M), -3.0), np.full((C, pr.M), -5.0)
    sd_N, sd_G = np.full((C, pr.M), 1.5), np.full((C, pr.M), 1.0)
    return postfilter.Model(np.full(C, 0.01), mu_N, sd_N, mu_G, sd_G, np.ones((C, pr.M), bool))


def test_ms_coef_agrees_with_hand_values():
    import postfilter
    m = _model()
    c = postfilter.ms_coef(m, 1.0)
    assert c.shape == (3, pr.M, 2) and c.dtype == np.float32
    assert not c[:, 0].any()                                          # g_0 = 1
    assert np.array_equal(c[:, 1:, 0], np.full((3, 32), 0.25, np.float32))            # 0.5 (1.5 - 1)
    assert np.array_equal(c[:, 1:, 1], np.full((3, 32), 2.25, np.float32))            # 0.5 (-3 + 1.5 * 5)
    c = postfilter.ms_coef(m, 0.5)
    assert np.array_equal(c[:, 1:, 0], np.full((3, 32), 0.125, np.float32)) and np.array_equal(c[:, 1:, 1], np.full((3, 32), 1.125, np.float32))
    assert not postfilter.ms_coef(m, 0.0).any()
    # a bin at the generated mean is moved to the natural mean: exp(a s + b) squared times e^s is e^mu_N
    a, b = postfilter.ms_coef(m, 1.0)[0, 5].astype(np.float64)
    assert abs(2.0 * (a * -5.0 + b) + -5.0 - -3.0) <= 1e-12
    with pytest.raises(ValueError):
        postfilter.ms_coef(m, 1.5)


def test_an_unusable_entry_gives_zero_coefficients(tmp_path):
    """model_from_stats on hand-made counts and sums: the mean and deviation come out, an entry seen in fewer than 2 segments
    on either side is unusable and its coefficients are 0; save and load keep every field."""
    import postfilter
    C = 2
    ms_n, ms_g = np.zeros((1, C, pr.M, 3)), np.zeros((2, C, pr.M, 3))
    ms_n[0, :, :] = [4.0, -8.0, 20.0]                                 # four values with sum -8, squares 20: mean -2, deviation 1
    ms_g[:, :, :] = [2.0, -6.0, 20.0]                                 # two utterances: mean -3, deviation 1
    ms_n[0, 1, 7] = [1.0, -2.0, 4.0]                                  # seen once on the natural side
    ms_g[:, 0, 9] = 0.0                                               # never seen on the generated side
    st = np.zeros((3, C, 2))
    st[:, :, 1] = [[0.01, 0.02], [0.03, 0.04], [9.0, 9.0]]
    m = postfilter.model_from_stats([(st, [50, 60, 0])], [ms_n], [ms_g])
    assert np.allclose(m.gv_t, [0.02, 0.03]) and m.mu_N[0, 3] == -2.0 and m.sd_N[0, 3] == 1.0 and m.mu_G[0, 3] == -3.0 and m.sd_G[0, 3] == 1.0
    assert not m.usable[1, 7] and not m.usable[0, 9] and m.usable.sum() == C * pr.M - 2
    c = postfilter.ms_coef(m, 1.0)
    assert not c[1, 7].any() and not c[0, 9].any() and c[0, 3].tolist() == [0.0, 0.5] and not c[:, 0].any()
    postfilter.save(str(tmp_path / 'm.npz'), m)
    back = postfilter.load(str(tmp_path / 'm.npz'))
    assert all(np.array_equal(getattr(back, f), getattr(m, f)) for f in postfilter.Model._fields)
    with pytest.raises(ValueError):
        postfilter.check_apply_args('both', 0.85, 1.0, 20.0, 4.0)
    with pytest.raises(ValueError):
        postfilter.check_apply_args('ms', 0.85, 1.0, -1.0, 4.0)


def test_float32_twin_stays_close_to_float64():
    x = _traj(8, 2, 129, 7)
    x *= np.float32(0.9 / np.abs(x).max())
    n = [129, 63]
    st = pr.traj_stats(x, n, np.float32)
    assert np.abs(st - pr.traj_stats(x, n)).max() <= 1e-7
    c = _coef(9, 7)
    assert np.abs(pr.ms_filter(x, n, st, c, -HI, HI, np.float32) - pr.ms_filter(x, n, st, c, -HI, HI)).max() <= 2e-6
    assert np.abs(pr.gv_filter(x, n, st, np.full(7, 0.02), 1.0, 4.0, np.float32) - pr.gv_filter(x, n, st, np.full(7, 0.02), 1.0, 4.0)).max() <= 5e-7


def test_entry_points_validate_on_the_host():
    """NULL pointers and bad scalars are VC_ERR_INVALID (1), sizes beyond the limits VC_ERR_UNSUPPORTED (4), both before any
    HIP call: none of these addresses is ever dereferenced, and no GPU is needed."""
    import _vc
    h = _vc.lib()
    P = ctypes.c_void_p(4096)
    ok = (2, 70, 5)
    stats = lambda x=P, st=P, shape=ok: h.vc_traj_stats_f32(x, None, *shape, st, None)
    gv = lambda x=P, st=P, t=P, y=ctypes.c_void_p(8192), shape=ok, alpha=1.0, g_max=4.0: h.vc_gv_filter_f32(x, None, st, t, *shape, alpha, g_max, y, None)
    mss = lambda x=P, st=P, o=P, shape=ok: h.vc_ms_stats_f32(x, None, st, *shape, o, None)
    msf = lambda x=P, st=P, c=P, y=ctypes.c_void_p(8192), shape=ok, lo=-1.0, hi=1.0: h.vc_ms_filter_f32(x, None, st, c, *shape, lo, hi, y, None)
    for call, names in ((stats, ('x', 'st')), (gv, ('x', 'st', 't', 'y')), (mss, ('x', 'st', 'o')), (msf, ('x', 'st', 'c', 'y'))):
        for name in names:
            assert call(**{name: None}) == 1, (call, name)
            assert b'NULL' in h.vc_last_error()
        for shape in ((0, 70, 5), (2, 0, 5), (2, 70, 0), (-1, 70, 5)):
            assert call(shape=shape) == 1, shape
        for shape in ((65536, 70, 5), (2, 16385, 5), (2, 70, 2050)):
            assert call(shape=shape) == 4, shape
            assert b'limits' in h.vc_last_error()
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float('nan')), dict(g_max=0.5), dict(g_max=float('inf')), dict(y=P)):
        assert gv(**kw) == 1, kw
    for kw in (dict(lo=0.1), dict(hi=-0.1), dict(lo=float('-inf')), dict(hi=float('nan')), dict(y=P)):
        assert msf(**kw) == 1, kw


def test_the_postfilter_kernels_spill_nothing():
    """Both modulation-spectrum kernels keep a 64-point transform per lane in registers; a change that tips them into scratch
    would still compute the right thing, several times slower.  The compiler's resource report says 0 spilled registers and 0
    bytes of scratch for all four kernels, and the committed report (profiles/postfilter/resource_usage.txt) says the same."""
    csrc = os.path.join(ROOT, 'speech-cloner_amd', 'csrc')
    out = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-fno-slp-vectorize', '-std=c++17', '--offload-arch=gfx950',
                          '--cuda-device-only', '-I', os.path.join(ROOT, 'include'), '-I', csrc, '-c',
                          os.path.join(csrc, 'vc_postfilter.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    committed = open(os.path.join(ROOT, 'profiles', 'postfilter', 'resource_usage.txt')).read()
    for report in (out.stderr, committed):
        blocks = report.split('Function Name:')
        for kern in ('traj_stats_kernel', 'gv_filter_kernel', 'ms_stats_kernel', 'ms_filter_kernel'):
            mine = [b for b in blocks if b.strip() and kern in b.splitlines()[0]]
            assert len(mine) == 1, 'no resource report for %s' % kern
            spill = re.search(r'VGPRs Spill: (\d+)', mine[0])
            sspill = re.search(r'SGPRs Spill: (\d+)', mine[0])
            scratch = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', mine[0])
            assert spill and int(spill.group(1)) == 0, (kern, mine[0])
            assert sspill and int(sspill.group(1)) == 0, (kern, mine[0])
            assert scratch and int(scratch.group(1)) == 0, (kern, mine[0])


def test_the_filter_undoes_over_smoothing_on_held_out_data():
    """seeded AR(1) trajectories, "generated" = smoothed by 0.2 / 0.6 / 0.2 along time and shrunk to 0.8
    of the deviation from the mean; the model fitted on 12 utterances, the filter (k = 1, max_db = 20, float64) applied to the
    6 others.  The caps are conditions on the definition, not measurements."""
    r = pr.experiment(k=1.0, max_db=20.0)
    print('MEASURED over-smoothing experiment: MS distance %.2f dB -> %.2f dB (natural held-out %.2f dB): ratios %.3f and %.3f; '
          'variance ratio %.3f -> %.3f; RMS error %.4f -> %.4f: ratio %.3f; clamped gains %.4f'
          % (r['d_gen'], r['d_out'], r['d_nat'], r['ms_ratio_gen'], r['ms_ratio_nat'], r['var_gen'], r['var_out'], r['e_gen'],
             r['e_out'], r['err_ratio'], r['clamped']))
    assert r['ms_ratio_gen'] <= 0.25
    assert r['ms_ratio_nat'] <= 2.0
    assert 0.8 <= r['var_out'] <= 1.1
    assert r['err_ratio'] <= 0.5
    assert r['clamped'] <= 0.01
