"""The reference of the pitch tracker with several candidates per frame (tests/f0_track_ref.py) pinned against itself and
against f0_ref, the host checks of evaluation.f0_candidates_batch / f0_viterbi_batch / f0_track_batch, and the three
entry points' declarations, bindings, exports and refusals.  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import f0_ref as fr
import f0_track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU_MIN, TAU_MAX = fr.lag_range(16000)
GLIDE_SEEDS, WEAK_SEEDS = (11, 12, 13, 14), (0, 1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def _signal(kind, seed):
    """(x, f0_true, voiced, yin f0, yin aperiodicity, candidates dict) of one test signal, float64, computed once."""
    x, f0_true, voiced = fr.glide_signal(seed) if kind == 'glide' else tr.weak_signal(seed)
    dp = tr.dprime(x)
    f0, ap = tr.yin_from_dprime(dp[0])
    return x, f0_true, voiced, f0, ap, tr.candidates(x, dp=dp)


ALL = [('glide', s) for s in GLIDE_SEEDS] + [('weak', s) for s in WEAK_SEEDS]


def test_yin_from_dprime_is_f0_ref_yin():
    x, _, _, f0, ap, _ = _signal('weak', 0)
    want_f0, want_ap = fr.yin(x)
    assert np.array_equal(f0, want_f0) and np.array_equal(ap, want_ap)


@pytest.mark.parametrize('kind,seed', ALL)
def test_candidates_contain_the_range_minimum(kind, seed):
    """A frame has a candidate exactly when its aperiodicity is below the ceiling, the lowest cost among its candidates IS
    the aperiodicity, lags ascend, and every candidate is a local minimum of d' below the ceiling."""
    c = _signal(kind, seed)[5]
    ap, n = c['aperiodicity'], c['n']
    assert np.array_equal(n > 0, ap < 1.0)
    for f in np.nonzero(n)[0]:
        lags, cost = c['lag'][f, :n[f]], c['cost'][f, :n[f]]
        assert cost.min() == ap[f] and (np.diff(lags) > 0).all() and TAU_MIN <= lags[0] and lags[-1] <= TAU_MAX
        row = c['dp'][f]
        for tau in lags:
            assert row[tau] < 1.0 and (tau == TAU_MIN or row[tau] < row[tau - 1]) and (tau == TAU_MAX or row[tau] <= row[tau + 1])
    assert (c['lag'][np.arange(8)[None, :] >= n[:, None]] == 0).all() and n.max() <= 8


def test_the_lowest_are_kept_and_a_tie_goes_to_the_smaller_lag():
    dp = np.ones((1, TAU_MAX + 2))
    dp[0, [50, 60, 70, 80, 90]] = [0.5, 0.25, 0.5, 0.25, 0.75]
    lags, n = tr.select(dp, TAU_MIN, TAU_MAX, 3, 1.0)
    assert n[0] == 3 and lags[0].tolist() == [50, 60, 80]                       # 0.25, 0.25, then the first 0.5
    lags, n = tr.select(dp, TAU_MIN, TAU_MAX, 8, 0.5)
    assert n[0] == 2 and lags[0].tolist() == [60, 80, 0, 0, 0, 0, 0, 0]         # the ceiling is strict
    dp[0, TAU_MIN], dp[0, TAU_MAX], dp[0, TAU_MAX + 1] = 0.9, 0.9, 0.1          # the range's ends: outside neighbours do not count
    assert tr.select(dp, TAU_MIN, TAU_MAX, 8, 1.0)[0][0].tolist() == [TAU_MIN, 50, 60, 70, 80, 90, TAU_MAX, 0]
    dp[0, 100:103] = 0.6                                                        # a plateau: its first lag (< left, <= right)
    assert tr.select(dp, TAU_MIN, TAU_MAX, 8, 1.0)[0][0].tolist() == [TAU_MIN, 50, 60, 70, 80, 90, 100, TAU_MAX]
    assert tr.select(np.ones((2, TAU_MAX + 2)), TAU_MIN, TAU_MAX, 8, 1.0)[1].tolist() == [0, 0]     # digital silence


@pytest.mark.parametrize('kind,seed', ALL)
def test_zero_transition_costs_reproduce_yin_voicing(kind, seed):
    _, _, _, f0, _, c = _signal(kind, seed)
    state, total = tr.viterbi(c['pitch'], c['cost'], c['n'], 0.15, 0.0, 0.0)
    assert np.array_equal(state > 0, f0 > 0)
    assert abs(total - np.minimum(c['aperiodicity'], 0.15).sum()) < 1e-9        # every frame pays its own cheapest state


@pytest.mark.parametrize('seed', WEAK_SEEDS)
def test_viterbi_removes_the_octave_errors_of_the_weak_fundamental(seed):
    """Frames more than 300 cents from the truth over f0_ref.fully_voiced_frames: the decoded track has at most a
    quarter of YIN's.  Measured: YIN 141, 110, 197, 118, 86, 116 of 292; Viterbi 7, 7, 0, 7, 0, 0."""
    x, f0_true, voiced, f0, _, c = _signal('weak', seed)
    got = tr.track(x, cand=c)[0]
    g_yin, scored = tr.gross_errors(f0, f0_true, voiced)
    g_vit, _ = tr.gross_errors(got, f0_true, voiced)
    print('seed %d: %d frames scored, gross errors YIN %d, Viterbi %d' % (seed, scored, g_yin, g_vit))
    assert scored == 292 and g_yin >= 40 and 4 * g_vit <= g_yin


def _lat(frames, n_cand):
    """frames: a list of [(pitch, cost), ...] per frame -> pitch, cost, n (unused slots: pitch 0, cost 0 -- cheap)."""
    F = len(frames)
    pitch, cost, n = np.zeros((F, n_cand), np.float32), np.zeros((F, n_cand), np.float32), np.zeros(F, np.int32)
    for f, cs in enumerate(frames):
        n[f] = len(cs)
        for k, (p, c) in enumerate(cs):
            pitch[f, k], cost[f, k] = p, c
    return pitch, cost, n


HAND = {
    # name: (lattice, (unvoiced, jump, switch), path, total)
    'tie_to_the_lower_state': (_lat([[(7.0, 0.25), (7.0, 0.25)]] * 3, 2), (1.0, 0.5, 0.5), [1, 1, 1], 0.75),
    'tie_between_unvoiced_and_voiced': (_lat([[(7.0, 0.5)]] * 2, 1), (0.5, 0.0, 0.0), [0, 0], 1.0),
    'tie_in_the_predecessor': (_lat([[(7.0, 0.25), (8.0, 0.25)], [(7.5, 0.0)]], 2), (2.0, 1.0, 1.0), [1, 1], 0.75),
    'an_absent_state_is_not_taken': (_lat([[(7.0, 0.5), (8.0, 0.5)], [(7.0, 0.5)], [(7.0, 0.5), (8.0, 0.0)]], 2), (1.0, 1.0, 1.0),
                                     [1, 1, 1], 1.5),
    'frames_without_candidates': (_lat([[(7.0, 0.0)], [], [], [(7.0, 0.0)]], 1), (0.25, 1.0, 0.125), [1, 0, 0, 1], 0.75),
    'one_frame': (_lat([[(7.0, 0.5), (8.0, 0.25), (9.0, 0.375)]], 3), (0.5, 1.0, 1.0), [2], 0.25),
    'one_frame_without_candidates': (_lat([[]], 4), (0.5, 1.0, 1.0), [0], 0.5),
    'the_octave_jump_costs_more_than_the_weaker_dip': (_lat([[(7.0, 0.25)], [(7.0, 0.5), (8.0, 0.25)], [(7.0, 0.25)]], 2),
                                                       (2.0, 0.5, 1.0), [1, 1, 1], 1.0),
    'staying_unvoiced_through_one_cheap_candidate': (_lat([[], [(7.0, 0.0)], []], 1), (0.125, 1.0, 0.5), [0, 0, 0], 0.375),
}


@pytest.mark.parametrize('name', sorted(HAND))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_hand_made_lattices(name, dtype):
    (pitch, cost, n), (uc, jc, sc), path, total = HAND[name]
    state, got = tr.viterbi(pitch, cost, n, uc, jc, sc, dtype)
    assert state.tolist() == path and got == total


@pytest.mark.parametrize('n_cand', [1, 8, 15])
def test_float32_restatement_equals_float64_on_dyadic_lattices(n_cand):
    rng = np.random.RandomState(100 + n_cand)
    for F in (1, 2, 3, 257, 2000):
        pitch, cost, n = tr.dyadic_lattice(rng, F, n_cand)
        uc, jc, sc = (rng.randint(0, 33, 3) / 16.0).tolist()
        s64, t64 = tr.viterbi(pitch, cost, n, uc, jc, sc)
        s32, t32 = tr.viterbi(pitch, cost, n, uc, jc, sc, np.float32)
        assert np.array_equal(s64, s32) and t64 == t32 and (s64 <= n).all()


def test_new_exports_are_declared_exported_and_bound():
    """Fails without the feature: the header, the binding and the library name the three entry points; the ABI stays 7."""
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    assert int(re.search(r'#define\s+VC_ABI_VERSION\s+(\d+)', hdr).group(1)) == 7 == _vc.VC_ABI_VERSION
    lib = _vc.lib()
    assert lib.vc_version() == 7
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, ret in (('vc_f0_candidates_f32', 'int'), ('vc_f0_viterbi_f32', 'int'), ('vc_f0_viterbi_workspace_size', 'size_t'),
                      ('vc_f0_viterbi_tile', 'int32_t')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), code), name
        assert name in _vc._SIGS and hasattr(lib, name)
    assert list(_vc._SIGS)[-2:] == ['vc_f0_yin_f32', 'vc_f0_metrics_f32']           # older names keep their places
    ws = lib.vc_f0_viterbi_workspace_size
    assert ws(3, 501, 8) == 3 * 501 * 8 and ws(65535, 2 ** 30 + 1, 15) == 65535 * (2 ** 30 + 1) * 8
    assert [ws(0, 10, 8), ws(65536, 10, 8), ws(1, 0, 8), ws(1, 2 ** 30 + 2, 8), ws(1, 10, 0), ws(1, 10, 16), ws(-1, 10, 8)] == [0] * 7
    assert lib.vc_f0_viterbi_tile() == 128


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """No GPU here: a refusal that came after a HIP call would report VC_ERR_HIP (2), not INVALID (1) / UNSUPPORTED (4)."""
    import _vc
    lib = _vc.lib()
    p = ctypes.c_void_p(4096)
    inf, nan = float('inf'), float('nan')

    def cand(wav=p, batch=2, max_len=80000, ld=80000, sr=16000.0, hop=80, W=512, tau_min=40, tau_max=267, ceiling=1.0, n_cand=8,
             f0=p, pitch=p, cost=p, n=p, ap=p, max_frames=1001):
        return lib.vc_f0_candidates_f32(wav, p, batch, max_len, ld, sr, hop, W, tau_min, tau_max, ceiling, n_cand, f0, pitch, cost, n,
                                        ap, max_frames, None)

    for kw in (dict(wav=None), dict(f0=None), dict(pitch=None), dict(cost=None), dict(n=None), dict(ap=None)):
        assert cand(**kw) == 1 and b'vc_f0_candidates_f32: NULL' in lib.vc_last_error(), kw
    for kw in (dict(batch=0), dict(max_len=0), dict(ld=79999), dict(hop=0), dict(W=0), dict(n_cand=0), dict(n_cand=-3)):
        assert cand(**kw) == 1 and b'vc_f0_candidates_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(tau_min=0), dict(tau_min=268)):
        assert cand(**kw) == 1 and b'tau_min <= tau_max' in lib.vc_last_error(), kw
    for kw in (dict(sr=0.0), dict(sr=inf), dict(ceiling=0.0), dict(ceiling=-1.0), dict(ceiling=inf), dict(ceiling=nan)):
        assert cand(**kw) == 1 and b'finite ceiling > 0' in lib.vc_last_error(), kw
    assert cand(max_frames=1000) == 1 and b'max_frames 1000 is less than' in lib.vc_last_error()
    for kw in (dict(batch=65536), dict(W=2049), dict(tau_max=1023), dict(hop=65537), dict(max_len=2 ** 30 + 1, ld=2 ** 30 + 1),
               dict(max_frames=2 ** 30 + 2), dict(n_cand=16)):
        assert cand(**kw) == 4 and b'vc_f0_candidates_f32: limits' in lib.vc_last_error(), kw

    def vit(pitch=p, cost=p, n=p, batch=2, F=501, n_cand=8, uc=0.15, jc=0.5, sc=0.1, cf0=p, state=p, f0=p, total=p, ws=p, nbytes=None):
        nbytes = 2 * 501 * 8 if nbytes is None else nbytes
        return lib.vc_f0_viterbi_f32(pitch, cost, n, p, batch, F, n_cand, uc, jc, sc, cf0, state, f0, total, ws, nbytes, None)

    for kw in (dict(pitch=None), dict(cost=None), dict(n=None), dict(state=None), dict(total=None), dict(ws=None)):
        assert vit(**kw) == 1 and b'vc_f0_viterbi_f32: NULL' in lib.vc_last_error(), kw
    for kw in (dict(cf0=None), dict(f0=None)):
        assert vit(**kw) == 1 and b'together' in lib.vc_last_error(), kw
    for kw in (dict(batch=0), dict(F=0), dict(n_cand=0)):
        assert vit(**kw) == 1 and b'vc_f0_viterbi_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(uc=-0.1), dict(uc=nan), dict(jc=inf), dict(jc=-1.0), dict(sc=nan), dict(sc=-0.5)):
        assert vit(**kw) == 1 and b'finite and not negative' in lib.vc_last_error(), kw
    for kw in (dict(batch=65536, nbytes=2 ** 40), dict(n_cand=16), dict(F=2 ** 30 + 2, nbytes=2 ** 40)):
        assert vit(**kw) == 4 and b'vc_f0_viterbi_f32: limits' in lib.vc_last_error(), kw
    assert vit(nbytes=2 * 501 * 8 - 1) == 1 and b'workspace of' in lib.vc_last_error()
    assert vit(ws=ctypes.c_void_p(4100)) == 1 and b'8-byte aligned' in lib.vc_last_error()


def test_python_checks_come_before_any_gpu_work():
    import torch
    import evaluation as ev
    wav = np.zeros((2, 4000), np.float32)
    lat = np.zeros((2, 51, 8), np.float32)
    n = np.zeros((2, 51), np.int32)
    bad = [lambda: ev.f0_candidates_batch(wav[0]), lambda: ev.f0_candidates_batch(torch.zeros(2, 40, dtype=torch.float64)),
           lambda: ev.f0_candidates_batch(wav, n_cand=0), lambda: ev.f0_candidates_batch(wav, n_cand=16),
           lambda: ev.f0_candidates_batch(wav, n_cand=2.0), lambda: ev.f0_candidates_batch(wav, ceiling=0.0),
           lambda: ev.f0_candidates_batch(wav, ceiling=float('nan')), lambda: ev.f0_candidates_batch(wav, [4000, 4001]),
           lambda: ev.f0_candidates_batch(wav, fmin=10.0), lambda: ev.f0_candidates_batch(wav, hop_length=0),
           lambda: ev.f0_track_batch(wav, threshold=0.0), lambda: ev.f0_track_batch(wav, jump_cost=-1.0),
           lambda: ev.f0_track_batch(wav, switch_cost=float('inf')), lambda: ev.f0_track_batch(wav, n_cand=True),
           lambda: ev.f0_track_batch(wav, [1]), lambda: ev.f0_track_batch(wav[0]),
           lambda: ev.f0_viterbi_batch(lat, lat[:, :50], n, [51, 51]), lambda: ev.f0_viterbi_batch(lat[0], lat[0], n, [51, 51]),
           lambda: ev.f0_viterbi_batch(lat, lat, n[:, :50], [51, 51]), lambda: ev.f0_viterbi_batch(lat, lat, n.astype(np.float32), [51, 51]),
           lambda: ev.f0_viterbi_batch(lat, lat, n, [51, 52]), lambda: ev.f0_viterbi_batch(lat, lat, n, [0, 51]),
           lambda: ev.f0_viterbi_batch(lat, lat, n, [51, 51], unvoiced_cost=-1.0), lambda: ev.f0_viterbi_batch(lat, lat, n, [51, 51], jump_cost=float('nan')),
           lambda: ev.f0_viterbi_batch(lat, lat, n, [51, 51], f0=lat[:, :, :4]),
           lambda: ev.f0_viterbi_batch(np.zeros((2, 51, 16), np.float32), np.zeros((2, 51, 16), np.float32), n, [51, 51]),
           lambda: ev.score_wav_batch(wav, [4000, 4000], wav, [4000, 4000], dict(sample_rate=16000), f0_method='pyin')]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    if not torch.cuda.is_available():                       # valid arguments reach the device check, and no further
        import _vc
        for call in (lambda: ev.f0_candidates_batch(wav), lambda: ev.f0_track_batch(wav, [4000, 1]),
                     lambda: ev.f0_viterbi_batch(lat, lat, n, [51, 1], f0=lat)):
            with pytest.raises(_vc.VCError, match='needs a GPU'):
                call()


def test_the_new_kernels_keep_their_registers():
    """The compiler's own report of the shipped compilation (the command `make -n` prints): no spills to scratch in
    f0_candidates_kernel (up to 1,024 lanes: 128 registers at most) and f0_viterbi_kernel, and the kernel f0_yin_kernel
    shares its d' with still has none."""
    import shlex
    import subprocess
    csrc = os.path.join(ROOT, 'speech-cloner_amd', 'csrc')
    for src, kerns in (('vc_f0', ('f0_yin_kernel', 'f0_candidates_kernel')), ('vc_f0_track', ('f0_viterbi_kernel',))):
        dry = subprocess.run(['make', '-C', csrc, '-n', '-B', src + '.o', 'ARCH=gfx950'], capture_output=True, text=True)
        assert dry.returncode == 0, dry.stderr
        line = [ln for ln in dry.stdout.splitlines() if src + '.hip' in ln and ' -c ' in ln]
        assert len(line) == 1, dry.stdout
        cmd = shlex.split(line[0])
        k = cmd.index('-o')
        cmd = cmd[:k] + cmd[k + 2:] + ['--cuda-device-only', '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage']
        out = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        blocks = out.stderr.split('Function Name:')
        for kern in kerns:
            mine = [b for b in blocks if kern in b.splitlines()[0]]
            assert mine, 'no resource report for %s' % kern
            assert int(re.search(r'VGPRs Spill: (\d+)', mine[0]).group(1)) == 0, mine[0]
            assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', mine[0]).group(1)) == 0, mine[0]
            assert int(re.search(r' VGPRs: (\d+)', mine[0]).group(1)) <= (128 if kern != 'f0_viterbi_kernel' else 256), mine[0]
