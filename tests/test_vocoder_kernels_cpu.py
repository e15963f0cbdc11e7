"""CPU half of the vocoder kernel tests: tests/vocoder_kernels_ref.py (what tests/test_vocoder_kernels_gpu.py holds the
kernels against) is itself held against oracle/vocoder_oracle.py and tests/fgla_ref.py, and the bounds it states are shown
to be able to fail: each is a small share of what it guards."""
import functools

import numpy as np
import pytest

import fgla_ref
import vocoder_kernels_cases as vc
import vocoder_kernels_ref as ref
from oracle import vocoder_oracle as vo

HANN = tuple(c for c in vc.ALL if vc.CASES[c][3] is None)
CUSTOM = tuple(c for c in vc.ALL if vc.CASES[c][3] is not None)
EPS = 1e-11             # float64 rounding through transforms of up to 4096 points, relative to the peak


def _exact_window(cid):
    n_fft, win, _, _ = vc.geometry(cid)
    return ref.padded_window(win, n_fft, vc.taps(cid))


def _close(a, b, tol=EPS):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= tol * scale, (float(np.abs(a - b).max()), scale)


@functools.lru_cache(maxsize=None)
def _history(cid, b, momentum, n):
    """Frames after every launch of the reference loop on utterance b (device window)."""
    amp, ph = vc.single(cid, b)
    keep = []
    ref.griffin_lim(amp, ph, vc.window(cid), vc.geometry(cid)[2], n, momentum, keep=keep)
    return keep


# ------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize('cid', HANN)
def test_reference_equals_the_oracle(cid):
    n_fft, win, hop, frames = vc.geometry(cid)
    w = _exact_window(cid)
    b = 2
    amp, ph = vc.single(cid, b)
    S0 = amp * np.exp(1j * ph)
    f1 = ref.frames_from_spectrum(S0, w)
    wav1 = ref.waveform(f1, w, hop)
    _close(wav1, vo.istft(S0.T, hop, win))
    _close(wav1, vo.griffin_lim_alg(amp.T, win, hop, num_iters=1, n_fft=n_fft, phase0=ph.T))
    # one and two float64 steps (the oracle's griffin_lim_step has no complex64 rounding); the projection's conditioning
    # multiplies float64 rounding, hence not EPS itself
    R, f2 = ref.step(f1, amp, w, hop)
    wav2 = ref.waveform(f2, w, hop)
    _close(wav2, vo.griffin_lim_step(wav1, amp.T, win, hop, n_fft), 1e-8)
    _close(ref.waveform(ref.griffin_lim(amp, ph, w, hop, 2), w, hop), wav2, 0.0)
    # the whole loop, plain and with momentum: the oracle's STFT stores complex64 like librosa's, so every spectrum it
    # projects is off by up to 2^-24 of each bin (as much of its norm); up to three projections follow, and a factor of 16
    # is left for what they make of it: 16 * 2^-24 of the waveform's norm.  (A wrong formula moves it by its own size.)
    for m, n in ((0.0, 3), (0.99, 4)):
        got = ref.waveform(ref.griffin_lim(amp, ph, w, hop, n, m), w, hop)
        want = fgla_ref.griffin_lim_momentum(amp.T, win, hop, n, m, n_fft=n_fft, phase0=ph.T)
        assert fgla_ref.rel_l2(got, want) <= 16 * ref.U, (cid, m, fgla_ref.rel_l2(got, want))
        if m == 0.0:
            _close(want, vo.griffin_lim_alg(amp.T, win, hop, num_iters=n, n_fft=n_fft, phase0=ph.T), 0.0)
    # a launch with momentum is the plain step on C = R - beta R_prev
    keep = _history(cid, b, 0.99, 4)
    wd = vc.window(cid)
    R1 = ref.analysis(keep[0], wd, hop)
    R2, f3 = ref.step(keep[1], amp, wd, hop, R1, ref.beta_of(0.99))
    _close(f3, keep[2], 0.0)
    assert abs(ref.beta_of(0.99) - 0.99 / 1.99) < 1e-7 and ref.beta_of(0.0) == 0.0


def test_unit_of_zero_is_phase_zero():
    u = ref.unit(np.array([0.0, -2.0, 3j, 0j]))
    assert np.array_equal(u, np.array([1.0, -1.0, 1j, 1.0]))
    assert np.array_equal(ref.project(np.array([0j, -4.0]), np.array([2.0, 3.0])), vo.project_phase(np.array([0j, -4.0]), np.array([2.0, 3.0])))


def test_dc_and_nyquist_imaginary_parts_are_ignored():
    rng = np.random.RandomState(0)
    S = rng.standard_normal((3, 9)) + 1j * rng.standard_normal((3, 9))
    w = ref.padded_window(12, 16)
    T = S.copy()
    T[:, 0] = T[:, 0].real
    T[:, -1] = T[:, -1].real
    full = np.concatenate([T, np.conj(T[:, -2:0:-1])], axis=1)
    _close(ref.frames_from_spectrum(S, w), np.fft.ifft(full, axis=1).real * w)


def test_overlap_add_keeps_the_sum_where_the_window_sum_is_zero():
    """hop == n_fft under the periodic Hann window: the window is exactly 0 at the frame joints, where the sum stays as it is."""
    w = ref.padded_window(400, 400)
    assert w[0] == 0.0 and ref.device_window(w)[0] == 0.0
    fr = np.ones((3, 400))
    y = ref.overlap_add(fr, w, 400)
    assert y[0] == y[400] == y[800] == 1.0 and np.allclose(y[1:400], 1.0 / w[1:] ** 2)
    assert np.array_equal(y, vo.window_sumsquare('hann', 3, 400, 400, 400) * 0 + y)
    wss = vo.window_sumsquare('hann', 3, 400, 400, 400)
    assert (wss[[0, 400, 800]] <= ref.F32_TINY).all() and (np.delete(wss, [0, 400, 800]) > ref.F32_TINY).all()


def test_inverse_preemphasis_and_power_to_amp_equal_the_oracle():
    rng = np.random.RandomState(1)
    x = rng.standard_normal(500)
    for c in (0.97, -0.97, 0.5, 0.0):
        _close(ref.inv_preemphasis(x, c), vo.calc_inv_preemphasis(x, c))
    y = ref.inv_preemphasis(x, 0.97)
    _close(ref.normalize(y, 0.045), y * (0.045 / np.abs(y).mean()))
    assert np.array_equal(ref.normalize(y, 0.0), y) and np.array_equal(ref.normalize(np.zeros(4), 0.1), np.zeros(4))
    P = rng.uniform(-0.2, 0.9, (7, 9))
    for r in (1.0, 1.25, 0.8):
        _close(ref.power_to_amp(P, 0.01, r), vo.power_to_amp(P, 0.01, r).T)
    assert np.isnan(ref.power_to_amp(-np.ones((2, 3)), 0.01, 1.25)).all()


# ------------------------------------------------------------------------------------------ windows, slots, sizes
@pytest.mark.parametrize('cid', CUSTOM + ('hop81', 'hop100-win320', 'n16'))
def test_perfect_reconstruction(cid):
    """istft(stft(y)) == y under the case's window: analysis and synthesis index the window the same way."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = _exact_window(cid)
    L = hop * (frames[2] - 1)
    y = np.random.RandomState(3).standard_normal(L)
    S = ref.stft_wave(y, w, hop)
    assert S.shape == (frames[2], ref.num_bins(n_fft))
    _close(ref.waveform(ref.frames_from_spectrum(S, w), w, hop), y, 1e-9)
    if cid in ('skew', 'skew16'):
        # the window is not symmetric, and reversing it in the analysis alone does not reconstruct
        assert np.abs(w - w[::-1]).max() > 0.2
        bad = ref.waveform(ref.frames_from_spectrum(ref.stft_wave(y, w[::-1].copy(), hop), w), w, hop)
        assert np.abs(bad - y).max() > 0.05 * np.abs(y).max()


def test_window_padding():
    w = ref.padded_window(12, 16)
    assert not w[:2].any() and not w[14:].any() and w[2] == 0.0 and w[3] > 0
    w = ref.padded_window(320, 400)
    assert not w[:40].any() and not w[360:].any() and np.count_nonzero(w) == 319
    assert np.array_equal(ref.padded_window(4, 4, [1, 2, 3, 4]), [1, 2, 3, 4])


def test_slot_map_is_the_hermitian_extension():
    k = ref.slot_bins400()
    assert k.shape == (13, 16) and len(np.unique(k)) == 208 and k.max() == 387 and k[3, 2] == 53
    rng = np.random.RandomState(2)
    R = rng.standard_normal((5, 201)) + 1j * rng.standard_normal((5, 201))
    R[:, 0] = R[:, 0].real
    R[:, 200] = R[:, 200].real
    full = np.fft.fft(np.fft.irfft(R, n=400, axis=1), axis=1)
    s = ref.slots_from_R400(R)
    _close(s, full[:, k])
    assert np.array_equal(s[:, 0, 9], np.conj(R[:, 175])) and np.array_equal(s[:, 12, 15], np.conj(R[:, 13]))
    amp = np.abs(R)
    assert np.array_equal(ref.slot_amp400(amp), np.abs(s))
    w = ref.padded_window(400, 400)
    _close(ref.frames_from_slots400(s, w), ref.frames_from_spectrum(R, w))


def test_restated_sizes():
    over = {c for c in vc.ALL if np.max(ref.lds_bytes(*vc.geometry(c)[:3:2])) > 64 * 1024}
    assert over == {'n2048', 'n4096'}
    assert ref.lds_bytes(4096, 1024) == 143392 <= 160 * 1024 < ref.lds_bytes(4096, 4096)
    assert ref.lds_bytes(400, 400) == (57152, 57280) and ref.lds_bytes(400, 80)[0] == 37952
    for c in vc.ALL:
        n_fft, win, hop, frames = vc.geometry(c)
        assert frames[0] == ref.min_frames(n_fft, hop) and hop * (frames[0] - 2) <= n_fft // 2 < hop * (frames[0] - 1)
        G = ref.tile_frames(n_fft)
        assert frames[1] % G == 1 and frames[1] > G and max(frames) == frames[2] and frames[2] % G
        assert max(frames) <= (10 if n_fft >= 2048 else 70)
    assert ref.nov_of(400, 81) == 5 and ref.nov_of(400, 7) == 58 and ref.nov_of(400, 400) == 1 and ref.nov_of(400, 200) == 2
    fb, o_wav, wb, o_state, total = ref.ws_layout(400, 80, 3, 37, 1, 1)
    assert (fb, o_wav, wb, o_state, total) == (177664, 355328, 34560, 424448, 424448 + 184832 + 256)       # 3 * 37 * 208 * 8 = 184,704
    assert ref.ws_layout(16, 5, 2, 7, 0, 0) == (1024, 2048, 0, 2048, 2304)


# ------------------------------------------------------------------------------------------ the bounds can fail
def _share(bound, guarded):
    return float(np.max(bound)) / float(np.max(np.abs(guarded)))


@pytest.mark.parametrize('cid', vc.ALL)
def test_linear_bounds_are_a_small_share_of_what_they_guard(cid):
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    worst = {}
    for b in range(len(frames) - 1):
        amp, ph = vc.single(cid, b)
        keep = _history(cid, b, 0.99, 5)
        for i, fr in enumerate(keep):
            # the spectrum whose frames these are has these magnitudes, and phases of no interest here: the analysis's own
            inv = ref.inverse_bound(ref.project(np.fft.rfft(fr, axis=1), amp), w)
            wav = ref.waveform(fr, w, hop)
            s = {'inverse': _share(inv, fr),
                 'overlap-add': _share(ref.trim(ref.ola_bound(fr, w, hop), n_fft), wav)}
            if i == 0:
                tot = ref.trim(ref.ola_of_bound(inv, w, hop) + ref.ola_bound(fr, w, hop), n_fft)
                s['initial waveform'] = _share(tot, wav)
            if i < len(keep) - 1:
                R = ref.analysis(fr, w, hop)
                s['forward'] = _share(ref.forward_bound(fr, w, hop), np.maximum(np.abs(R.real), np.abs(R.imag)))
            for k, v in s.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print('SHARES %s: %s' % (cid, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    assert all(0.0 < v < 1e-3 for v in worst.values()), (cid, worst)


@pytest.mark.parametrize('cid', vc.ALL)
def test_plain_cap_membership(cid):
    """Which cases take the plain late-iteration check: those whose model of one projection, from the reference's own
    frames alone, stays under PLAIN_CAP of the frames' peak at both iterations tested.  Every 400-point case must."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    worst = 0.0
    for b in range(len(frames) - 1):
        amp, _ = vc.single(cid, b)
        keep = _history(cid, b, 0.0, 5)
        for n in (3, 5):
            out, bound = ref.plain_step_bound(keep[n - 2], amp, w, hop)
            _close(out, keep[n - 1], 0.0)
            worst = max(worst, _share(bound, out))
    print('CAP %s: model / peak %.3e (cap %.1e)' % (cid, worst, ref.PLAIN_CAP))
    assert (worst <= ref.PLAIN_CAP) == (cid in vc.IN_CAP), (cid, worst)
    assert set(vc.POINT400) <= set(vc.IN_CAP)


def test_other_bounds_are_small_shares():
    rng = np.random.RandomState(4)
    x = rng.standard_normal(4097) * 0.1
    for c in (0.97, -0.97, 0.5, 0.0):
        y = ref.inv_preemphasis(x, c)
        yb = ref.inv_preemphasis_bound(x, c)
        assert 0 < _share(yb, y) < 1e-3
        assert 0 < _share(ref.normalize_bound(y, yb, 0.045), ref.normalize(y, 0.045)) < 1e-3
    P = rng.uniform(-0.1, 0.9, (37, 201))
    for r in (1.0, 1.25, 0.8):
        assert 0 < ref.power_to_amp_rel_bound(P, 0.01, r).max() < 1e-3
    assert ref.block_sum_terms(4097) == 5 + 16 and ref.block_sum_terms(5) == 17
