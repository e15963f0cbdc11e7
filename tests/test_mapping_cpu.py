"""Spectral mapping without a GPU: the numpy restatement of tests/mapping_ref.py against independent definitions (a dense
solve, EM's monotonicity, a seeded corpus), the float32 control against every derived bound on the inputs of the GPU tests,
the gain's interpolation table for the shipped front-end, and the argument checks of mapping.py and
conversion.convert_gmm_diff_batch, all of which are raised before any launch."""
import numpy as np
import pytest

import mapping_cases as mc
import mapping_ref as mr
import speaker_ref

TWIN_FRACTION = 0.5         # the float32 twin must stay below this fraction of every derived bound


@pytest.mark.parametrize('F', mc.SOLVE_FRAMES)
def test_banded_solve_equals_a_dense_solve(F):
    """The restatement's banded LDL^T against np.linalg.solve of the explicitly built A, b: 1e-12 relative."""
    n = 3
    P, R = mc.mlpg_case(n, [F], seed=F)
    y, flag = mr.mlpg(P[0], R[0], F)
    y64 = mlpg_float64_unrounded(P[0], R[0], F)
    A, b = mr.mlpg_system(P[0], R[0], F)
    want = np.stack([np.linalg.solve(A[j], b[j]) for j in range(n)], 1)
    for j in range(n):
        assert np.allclose(A[j], A[j].T) and np.linalg.eigvalsh(A[j]).min() > 0
        i, k = np.nonzero(A[j])
        assert np.abs(i - k).max(initial=0) <= 4
    rel = np.abs(y64 - want).max() / np.abs(want).max()
    print('MEASURED banded solve F=%d: relative error %.2e' % (F, rel))
    assert flag == 0 and rel <= 1e-12
    assert np.array_equal(y[:F], y64.astype(np.float32)) and not y[F:].any()


def mlpg_float64_unrounded(P, R, F):
    """mr.mlpg's trajectory before its one rounding: the same recurrences with a float64 output."""
    A, b = mr.mlpg_system(P, R, F)
    n = len(A)
    out = np.zeros((F, n))
    for j in range(n):
        # banded LDL^T by rows on the dense matrix: the recurrence of the header with exact zero terms left out
        L, d, z = np.eye(F), np.zeros(F), np.zeros(F)
        for i in range(F):
            v = {}
            for k in range(max(i - 4, 0), i):
                v[k] = A[j][i, k] - sum(v[p] * L[k, p] for p in range(max(i - 4, 0), k))
                L[i, k] = v[k] / d[k]
            d[i] = A[j][i, i] - sum(v[k] * L[i, k] for k in v)
            z[i] = b[j][i] - sum(L[i, k] * z[k] for k in range(max(i - 4, 0), i))
        y = np.zeros(F)
        for i in range(F - 1, -1, -1):
            y[i] = z[i] / d[i] - sum(L[k, i] * y[k] for k in range(i + 1, min(i + 5, F)))
        out[:, j] = y
    return out


def test_mlpg_flag_and_fallback_on_a_non_positive_precision():
    P, R = mc.mlpg_case(2, [9])
    P[0, 3, 0] = -40.0                                               # Ps of dimension 0: a pivot turns negative
    y, flag = mr.mlpg(P[0], R[0], 9)
    good, _ = mr.mlpg(*[a[0][:, [1, 3]] for a in (P, R)], 9)
    want = (R[0, :9, 0].astype(np.float64) / P[0, :9, 0].astype(np.float64)).astype(np.float32)
    assert flag == 1 and np.array_equal(y[:9, 0], want) and np.array_equal(y[:, 1], good[:, 0])


def test_mlpg_reproduces_a_trajectory_it_was_given():
    """Statics and deltas of a known trajectory as means under any positive precisions: the minimiser is the trajectory."""
    rng = np.random.RandomState(4)
    F, n = 46, 2
    y = rng.standard_normal((F, n)).astype(np.float32)
    E = speaker_ref.features(y, F, None, True, False)
    P = rng.uniform(0.5, 5.0, (F, 2 * n)).astype(np.float32)
    got, flag = mr.mlpg(P, (P.astype(np.float64) * E).astype(np.float32), F)
    assert flag == 0 and np.abs(got - y).max() <= 1e-5


@pytest.fixture(scope='module')
def corpus():
    xs, ys = mr.cepstral_corpus()
    X, lens = mr.batch(xs)
    Y, _ = mr.batch(ys)
    return X, Y, lens


def test_em_trace_rho_max_and_floors(corpus):
    X, Y, lens = corpus
    fa, fb = mr.features_batch(X, lens), mr.features_batch(Y, lens)
    model, trace = mr.fit(fa[:8], fb[:8], lens[:8], lens[:8], n_components=8, n_iter=12, var_floor=1e-2, rho_max=0.5)
    assert np.isfinite(trace).all() and (np.diff(trace) >= -1e-9).all(), trace
    st = mr.accumulate(*mr.gather(fa[:8], fb[:8], lens[:8], lens[:8]), dict(w=np.ones(1), mu_x=np.zeros((1, 8)), mu_y=np.zeros((1, 8)),
                       var_x=np.ones((1, 8)), var_y=np.ones((1, 8)), cov_xy=np.zeros((1, 8))))
    gx = st['S'][2, 0] / st['N'][0] - (st['S'][0, 0] / st['N'][0]) ** 2
    assert (model['var_x'] >= np.float32(1e-2) * gx.astype(np.float32) * (1 - 1e-6)).all()
    rho = model['cov_xy'].astype(np.float64) / np.sqrt(model['var_x'].astype(np.float64) * model['var_y'])
    assert np.abs(rho).max() <= 0.5 * (1 + 1e-6) and np.abs(rho).max() >= 0.5 * (1 - 1e-6)       # the clamp is reached here
    assert (model['var_x'].astype(np.float64) * model['var_y'] - model['cov_xy'].astype(np.float64) ** 2 > 0).all()
    assert abs(float(model['w'].sum()) - 1.0) < 1e-5


def test_a_starved_component_keeps_its_parameters():
    model = mr.random_model(3, 4, seed=2)
    N = np.array([5.0, 0.5, 0.0])
    S = np.random.RandomState(0).standard_normal((5, 3, 4))
    S[2:4] = np.abs(S[2:4]) + 3.0
    out = mr.update(N, S, model, np.full(4, 1e-3), np.full(4, 1e-3), 0.99, 1.0)
    for k in mr.FIELDS[1:]:
        assert np.array_equal(out[k][1:], model[k][1:]) and not np.array_equal(out[k][0], model[k][0])
    assert out['w'][2] == np.float32(2.0 ** -40) and abs(float(out['w'][0]) - 5.0 / 5.5) < 1e-6


def test_held_out_error_falls_and_mlpg_is_not_worse_than_mmse(corpus):
    X, Y, lens = corpus
    fa, fb = mr.features_batch(X, lens), mr.features_batch(Y, lens)
    model, _ = mr.fit(fa[:8], fb[:8], lens[:8], lens[:8], n_components=8, n_iter=20)
    n = X.shape[2]
    e0 = e_mmse = e_mlpg = cnt = 0.0
    for b in (8, 9):
        F = lens[b]
        P, R, mmse, _, _ = mr.map_stats(fa[b, :F], model)
        y, flag = mr.mlpg(P.astype(np.float32), R.astype(np.float32), F)
        assert flag == 0
        e0 += ((X[b, :F] - Y[b, :F]) ** 2).sum()
        e_mmse += ((mmse[:, :n] - Y[b, :F]) ** 2).sum()
        e_mlpg += ((y[:F] - Y[b, :F]) ** 2).sum()
        cnt += F * n
    r0, r1, r2 = (float(np.sqrt(e / cnt)) for e in (e0, e_mmse, e_mlpg))
    print('MEASURED held-out rms error: unconverted %.3f, MMSE %.3f, MLPG %.3f' % (r0, r1, r2))
    assert r1 < r0 and r2 < r0 and r2 <= r1 * (1 + 1e-6)


@pytest.mark.parametrize('M,D', mc.JD_SHAPES)
def test_the_float32_twin_stays_inside_the_cell_and_statistics_bounds(M, D):
    worst = 0.0
    for with_path in (True, False):
        model, fa, fb, la, lb, path, plen = mc.acc_case(M, D, with_path)
        x, y = mr.gather(fa, fb, la, lb, path, plen)
        assert len(x) > 0 and np.isfinite(x).all() and np.isfinite(y).all()          # no skipped cell was gathered
        ll64, E, _ = mr.joint_ll(x, y, model)
        ll32, _, _ = mr.joint_ll(x, y, model, np.float32)
        worst = max(worst, float((np.abs(ll32 - ll64) / mr.cell_bound(D, M, E)).max()))
        a, t = mr.accumulate(x, y, model), mr.accumulate(x, y, model, np.float32)
        d, tiny = a['delta'], 1e-300
        worst = max(worst, float((np.abs(t['N'] - a['N']) / (2 * d * a['N'] + tiny)).max()),
                    float((np.abs(t['S'] - a['S']) / (2 * d * a['A'] + tiny)).max()), abs(t['L'][0] - a['L'][0]) / (d * a['L'][1]))
        assert t['L'][1] == a['L'][1] == len(x)
    print('MEASURED float32 twin, E-step M=%d D=%d: %.3f of the bounds' % (M, D, worst))
    assert worst <= TWIN_FRACTION


@pytest.mark.parametrize('M,D', mc.JD_SHAPES)
@pytest.mark.parametrize('mixture', ['soft', 'best'])
def test_the_float32_twin_stays_inside_the_map_bounds_and_no_frame_is_left_out(M, D, mixture):
    model, feat, lens = mc.map_case(M, D)
    x = np.concatenate([feat[b, :l] for b, l in enumerate(lens)])
    P, R, E, best, bd = mr.map_stats(x, model, mixture)
    p, r, e, b32, _ = mr.map_stats(x, model, mixture, np.float32)
    assert (bd['margin'] > 2 * bd['delta_best']).all(), 'a frame would be left out of the arg-max comparison'
    assert np.array_equal(best, b32)
    worst = max(float((np.abs(p - P) / bd['P']).max()), float((np.abs(r - R) / bd['R']).max()), float((np.abs(e - E) / bd['mmse']).max()))
    print('MEASURED float32 twin, map %s M=%d D=%d: %.3f of the bounds' % (mixture, M, D, worst))
    assert worst <= TWIN_FRACTION


def test_the_interpolation_table_of_the_shipped_front_end():
    import audio_lib
    import mapping
    fb = audio_lib.host_tables(16000, 400, 80, 1)[0]
    nz = [np.flatnonzero(fb[:, k] > 0) for k in range(fb.shape[1])]
    assert [k for k in range(201) if len(nz[k]) == 0] == [0, 200]
    assert all(len(v) <= 2 and (len(v) < 2 or v[1] == v[0] + 1) for v in nz)
    i0, w = mapping.gain_tables(mc.CFG)
    r0, rw = mr.bin_table(fb)
    assert np.array_equal(i0, r0) and np.array_equal(w, rw) and i0.dtype == np.int32 and w.dtype == np.float32
    assert (i0 >= 0).all() and (i0 <= 78).all() and (w >= 0).all() and (w <= 1).all()
    assert (i0[0], w[0]) == (0, 0.0) and (i0[200], w[200]) == (78, 1.0)
    for k in range(1, 200):
        col = fb[:, k] / fb[:, k].sum()
        back = np.zeros(80)
        back[i0[k]] += 1.0 - w[k]
        back[i0[k] + 1] += w[k]
        assert np.abs(back - col).max() <= 1e-6
    bad = fb.copy()
    bad[5, 100] = 0.1                                                # a third, distant band on one bin
    with pytest.raises(ValueError, match='adjacent'):
        mapping.bin_table(bad)
    assert mapping.db_scale(mc.CFG) == 50.0


def test_host_arithmetic_of_the_library_matches_the_restatement():
    import _vc
    lib = _vc.lib()
    assert lib.vc_jd_tile() == mc.TILE == mr.TILE
    for M, D in mc.JD_SHAPES:
        assert lib.vc_jd_table_floats(M, D) == mr.table_floats(M, D)
        assert lib.vc_jd_workspace_size(M, D) == mr.workspace_size(M, D)
    assert lib.vc_jd_table_floats(257, 2) == 0 and lib.vc_jd_workspace_size(2, 65) == 0 and lib.vc_jd_workspace_size(0, 2) == 0
    assert lib.vc_mlpg_workspace_size(16, 1001, 24) == mr.mlpg_workspace_size(16, 1001, 24)
    assert lib.vc_mlpg_workspace_size(1, 1, 33) == 0 and lib.vc_mlpg_workspace_size(0, 1, 1) == 0
    # argument validation happens before any HIP call
    assert lib.vc_jd_prepare_f32(None, None, None, None, None, None, 2, 2, None, None) == 1 and b'vc_jd_prepare_f32' in lib.vc_last_error()
    assert lib.vc_mlpg_f32(None, None, None, 1, 1, 1, None, None, None, 0, None) == 1
    assert lib.vc_cep_gain_f32(None, None, None, 1, 1, 1, None, 80, None, None, 201, 1.0, 50.0, 20.0, 30.0, None, None) == 1


def test_argument_errors_are_raised_before_any_launch(corpus):
    import conversion
    import mapping
    X, Y, lens = corpus
    fa, fb = mr.features_batch(X, lens), mr.features_batch(Y, lens)
    m = mr.random_model(4, 8)
    model = mapping.JDGMM(*(m[k] for k in mr.FIELDS))
    wav = np.zeros((2, 4000), np.float32)
    path, plen = np.zeros((10, 50, 2), np.int32), np.full(10, 50, np.int32)
    bad = [
        (lambda: mapping.fit(fa, lens, fb[:, :, :6], lens), 'agree'),
        (lambda: mapping.fit(fa, lens, fb[0], lens), 'feat_tgt'),
        (lambda: mapping.fit(fa.astype(np.float64), lens, fb, lens), 'float32'),
        (lambda: mapping.fit(fa, lens, fb, [0] * 10), 'lens_tgt'),
        (lambda: mapping.fit(fa, lens, fb, lens, path=path), 'together'),
        (lambda: mapping.fit(fa, lens, fb, lens, path=path.astype(np.int64), path_len=plen), 'int32'),
        (lambda: mapping.fit(fa, lens, fb, lens, path=path[:, :, :1], path_len=plen), 'max_path'),
        (lambda: mapping.fit(fa, lens, fb, lens, n_components=257), 'n_components'),
        (lambda: mapping.fit(fa, lens, fb, lens, n_iter=0), 'n_iter'),
        (lambda: mapping.fit(fa, lens, fb, lens, var_floor=0.0), 'var_floor'),
        (lambda: mapping.fit(fa, lens, fb, lens, rho_max=1.0), 'rho_max'),
        (lambda: mapping.fit(fa, lens, fb, lens, min_count=-1.0), 'min_count'),
        (lambda: mapping.fit_wav(wav, None, wav, None, None), 'cfg_d'),
        (lambda: mapping.fit_wav(wav, None, wav[:1], None, mc.CFG), 'same number'),
        (lambda: mapping.fit_wav(wav, None, wav, None, mc.CFG, n_coef=33), 'coefficients'),
        (lambda: mapping.fit_wav(wav, None, wav, None, mc.CFG, n_realign=-1), 'n_realign'),
        (lambda: mapping.map_batch(model, fa, lens, mixture='hard'), 'mixture'),
        (lambda: mapping.map_batch(model[:5], fa, lens), 'JDGMM'),
        (lambda: mapping.map_batch(model, fa[:, :, :6], lens), r'\[M, D\]'),
        (lambda: mapping.mlpg_batch(fa[:, :, :7], fa[:, :, :7], lens), 'even'),
        (lambda: mapping.mlpg_batch(fa, fb[:, :5], lens), 'like P'),
        (lambda: mapping.convert_cepstra_batch(model, X[:, :, :3], lens), r'\[M, D\]'),
        (lambda: mapping.convert_cepstra_batch(model, X, [0] * 10), 'lens'),
        (lambda: mapping.cepstra_gain_batch(X, Y[:, :5], None, mc.CFG), 'same shape'),
        (lambda: mapping.cepstra_gain_batch(X, Y, None, mc.CFG, alpha=2.0), 'alpha'),
        (lambda: mapping.cepstra_gain_batch(X, Y, [99] * 10, mc.CFG), 'n_frames'),
        (lambda: mapping.cepstra_gain_batch(X, Y, None, None), 'cfg_d'),
        (lambda: conversion.convert_gmm_diff_batch(model, wav), 'cfg_d'),
        (lambda: conversion.convert_gmm_diff_batch(model[:3], wav, cfg_d=mc.CFG), 'JDGMM'),
        (lambda: conversion.convert_gmm_diff_batch(model, wav, cfg_d=mc.CFG, mixture='x'), 'mixture'),
        (lambda: conversion.convert_gmm_diff_batch(model, wav, cfg_d=mc.CFG, n_coef=5), 'n_coef'),
        (lambda: conversion.convert_gmm_diff_batch(model, wav, lens=[4000, 100], cfg_d=mc.CFG), 'n_fft//2'),
        (lambda: conversion.convert_gmm_diff_batch(model, wav, cfg_d=mc.CFG, max_cut_db=-1.0), 'max_cut_db'),
        (lambda: conversion.convert_gmm_diff_batch(model, wav, cfg_d=mc.CFG, denoise='yes'), 'denoise'),
    ]
    for call, pat in bad:
        with pytest.raises(ValueError, match=pat):
            call()


def test_the_kernels_keep_their_accumulators_in_registers():
    """The E-step holds 40 float64 sums and N per lane: the compiler's own resource report must say 0 spilled registers (vector
    and scalar: a per-dimension predicate once cost 21 scalar ones) and 0 scratch for every kernel of csrc/vc_mapping.hip."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, 'speech-cloner_amd', 'csrc')
    out = subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-fno-slp-vectorize', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only',
                          '-I', os.path.join(ROOT, 'include'), '-I', csrc, '-c', os.path.join(csrc, 'vc_mapping.hip'), '-o', os.devnull,
                          '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = out.stderr.split('Function Name:')[1:]
    names = ('jd_prepare_kernel', 'jd_accumulate_kernel', 'jd_reduce_kernel', 'jd_update_kernel', 'jd_map_kernel', 'mlpg_kernel',
             'cep_gain_kernel')
    for k in names:
        mine = [b for b in blocks if k in b.splitlines()[0]]
        assert mine, 'no resource report for %s' % k
        for what in (r'VGPRs Spill: (\d+)', r'SGPRs Spill: (\d+)', r'ScratchSize \[bytes/lane\]: (\d+)'):
            m = re.search(what, mine[0])
            assert m and int(m.group(1)) == 0, (k, what, mine[0])
