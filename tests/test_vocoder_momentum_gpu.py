"""GPU checks of fast Griffin-Lim (csrc/vc_vocoder.hip MOM flavours through vc_griffin_lim_momentum_f32)
against the CPU reference tests/fgla_ref.py.

Momentum extrapolates, so float32 differences grow faster than in the plain loop.  Parity bounds are
therefore not fixed numbers: a device run must stay within 3x the distance (relative L2) between the
reference's own float32 and float64 runs of the same input.  The generic path sums its direct DFTs of
N terms in float32 and is already several times further from float64 than an FFT at momentum 0 (the
plain algorithm, unchanged here); there the yardstick is the larger of that distance and the device's
own momentum-0 distance at the same iteration count, so the check still asks that momentum add no
error beyond what it adds in the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import fgla_ref as fr
from oracle import frontend_oracle as fo
from oracle import vocoder_oracle as vo

pytestmark = pytest.mark.gpu

ALPHA = 0.99


def _amp_of_speech(L, seed, n_fft=400, hop=80, win=400):
    y = fo.synth_speech(1, L, seed=seed)[0].astype(np.float64)
    y = y[:hop * (len(y) // hop)]
    return np.abs(vo.stft(y, n_fft, hop, win)).astype(np.float64)          # [bins, F]


def _device(amp, win, hop, n, m, ph, n_fft=None, verbose=False):
    import audio_lib
    return audio_lib.griffin_lim_alg(amp, win, hop, num_iters=n, n_fft=n_fft, verbose=verbose, phase0=ph, momentum=m)


def _ref_gap(amp, win, hop, n, m, ph, n_fft=None):
    r64 = fr.griffin_lim_momentum(amp, win, hop, n, m, n_fft=n_fft, phase0=ph)
    r32 = fr.griffin_lim_momentum(amp, win, hop, n, m, n_fft=n_fft, phase0=ph, dtype=np.float32)
    return r64, fr.rel_l2(r32, r64)


@pytest.mark.parametrize('n_iter', [3, 4, 8])
def test_parity_400_point_path(n_iter):
    amp = _amp_of_speech(8000, 11)
    ph = vo.initial_phase(amp.shape, 3)
    ref, gap = _ref_gap(amp, 400, 80, n_iter, ALPHA, ph)
    got = _device(amp, 400, 80, n_iter, ALPHA, ph)
    assert got.dtype == np.float32 and got.shape == ref.shape == (80 * (amp.shape[1] - 1),)
    assert 0.0 < gap and fr.rel_l2(got, ref) <= 3.0 * gap, (fr.rel_l2(got, ref), gap)
    # the momentum acted: the plain loop lands elsewhere
    assert fr.rel_l2(_device(amp, 400, 80, n_iter, 0.0, ph), ref) > 100.0 * gap


@pytest.mark.parametrize('n_iter', [3, 8])
@pytest.mark.parametrize('n_fft,win,hop,L', [(800, 800, 40, 4000), (512, 400, 128, 6400)])
def test_parity_generic_path(n_fft, win, hop, L, n_iter):
    """The sizes of test_vocoder_gpu.py::test_generic_transform_sizes."""
    amp = _amp_of_speech(L, 8, n_fft, hop, win)
    ph = vo.initial_phase(amp.shape, 4)
    ref, gap = _ref_gap(amp, win, hop, n_iter, ALPHA, ph, n_fft)
    got = _device(amp, win, hop, n_iter, ALPHA, ph, n_fft)
    plain_ref = fr.griffin_lim_momentum(amp, win, hop, n_iter, 0.0, n_fft=n_fft, phase0=ph)
    plain_gap = fr.rel_l2(_device(amp, win, hop, n_iter, 0.0, ph, n_fft), plain_ref)
    assert got.shape == ref.shape
    assert fr.rel_l2(got, ref) <= 3.0 * max(gap, plain_gap), (fr.rel_l2(got, ref), gap, plain_gap)


@pytest.mark.parametrize('n_fft,win,hop,L', [(400, 400, 80, 8000), (800, 800, 40, 4000)])
def test_first_projection_ignores_momentum_bit_for_bit(n_fft, win, hop, L):
    amp = _amp_of_speech(L, 2, n_fft, hop, win)
    ph = vo.initial_phase(amp.shape, 6)
    for n in (1, 2):
        base = _device(amp, win, hop, n, 0.0, ph, n_fft)
        for m in (0.5, ALPHA):
            assert np.array_equal(_device(amp, win, hop, n, m, ph, n_fft), base)


def _abi_run(entry, amp, ph, n, momentum=None, trace=False):
    """One call of vc_griffin_lim_f32 / vc_griffin_lim_momentum_f32 on [1, F, 201] tensors; returns (rc, wav)."""
    import _vc
    import audio_lib
    lib = _vc.lib()
    plan = audio_lib._get_voc_plan(400, 80, None)
    a = torch.from_numpy(np.ascontiguousarray(amp.T, dtype=np.float32))[None].cuda()
    p = torch.from_numpy(np.ascontiguousarray(ph.T, dtype=np.float32))[None].cuda()
    F = a.shape[1]
    L = 80 * (F - 1)
    wav = torch.full((1, L), 7.0, device='cuda')
    tr = torch.zeros((n, 1), device='cuda') if trace else None
    need = lib.vc_vocoder_workspace_bytes_momentum(plan.handle, 1, F, int(trace))
    assert need > lib.vc_vocoder_workspace_bytes(plan.handle, 1, F, int(trace))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    args = [plan.handle, _vc.ptr(a), _vc.ptr(p), None, 1, F, n]
    if momentum is not None:
        args.append(C.c_float(momentum))
    rc = getattr(lib, entry)(*args, _vc.ptr(wav), L, _vc.ptr(tr), _vc.ptr(ws), ws.numel(), _vc.current_stream())
    torch.cuda.synchronize()
    return rc, wav.cpu().numpy()[0]


def test_zero_momentum_entry_is_the_plain_entry_bit_for_bit():
    amp = _amp_of_speech(8000, 11)
    ph = vo.initial_phase(amp.shape, 3)
    for n in (1, 3, 8):
        rc0, plain = _abi_run('vc_griffin_lim_f32', amp, ph, n)
        rc1, zero = _abi_run('vc_griffin_lim_momentum_f32', amp, ph, n, 0.0)
        assert rc0 == rc1 == 0 and np.array_equal(plain, zero)
    rc2, mom = _abi_run('vc_griffin_lim_momentum_f32', amp, ph, 8, ALPHA)
    assert rc2 == 0 and not np.array_equal(mom, plain)


def test_bad_momentum_through_the_abi_is_an_error_not_a_launch():
    import _vc
    amp = _amp_of_speech(8000, 11)
    ph = vo.initial_phase(amp.shape, 3)
    for bad in (-0.25, 1.0, 2.0, float('nan'), float('inf')):
        rc, wav = _abi_run('vc_griffin_lim_momentum_f32', amp, ph, 4, bad)
        assert rc == 1 and b'momentum' in _vc.lib().vc_last_error(), (bad, rc)
        assert (wav == 7.0).all()                                            # nothing was launched
    # the bound itself: just under 1 is accepted
    rc, wav = _abi_run('vc_griffin_lim_momentum_f32', amp, ph, 4, float(np.nextafter(np.float32(1), np.float32(0))))
    assert rc == 0 and np.isfinite(wav).all()


def test_ragged_batch_equals_single_utterances_with_momentum():
    import audio_lib
    rng = np.random.RandomState(0)
    frames = [37, 120, 64]
    Fmax = max(frames)
    amp = np.zeros((3, Fmax, 201), np.float32)
    ph = np.zeros((3, Fmax, 201), np.float32)
    for b, F in enumerate(frames):
        amp[b, :F] = _amp_of_speech(80 * (F - 1), 20 + b).T
        ph[b, :F] = rng.uniform(0, np.pi, (F, 201))
    amp[1, 100:] += 7.0                      # garbage beyond n_frames must not leak in
    wav = audio_lib.griffin_lim_batch(amp, [37, 100, 64], 400, 80, num_iters=8, phase0=ph, momentum=ALPHA)
    wav = wav.cpu().numpy()
    for b, F in enumerate([37, 100, 64]):
        single = audio_lib.griffin_lim_batch(amp[b:b + 1, :F], None, 400, 80, num_iters=8, phase0=ph[b:b + 1, :F],
                                             momentum=ALPHA).cpu().numpy()[0]
        assert np.array_equal(wav[b, :80 * (F - 1)], single)                 # bit-identical
        assert not wav[b, 80 * (F - 1):].any()


@pytest.mark.parametrize('seed', [3, 7])
def test_convergence_on_the_device(seed):
    """test_vocoder_momentum_cpu.py's inputs: the device reaches the reference's spectral convergence
    and the same gain over its own 200 plain iterations."""
    amp = _amp_of_speech(24000, seed)
    ph = vo.initial_phase(amp.shape, 0)
    sc = {}
    for m, n in ((0.0, 200), (ALPHA, 32), (ALPHA, 50)):
        sc[(m, n)] = fr.sc(_device(amp, 400, 80, n, m, ph), amp, 400, 80)
    for n in (32, 50):
        ref = fr.sc(fr.griffin_lim_momentum(amp, 400, 80, n, ALPHA, phase0=ph), amp, 400, 80)
        assert abs(sc[(ALPHA, n)] - ref) <= 0.02 * ref, (n, sc[(ALPHA, n)], ref)
    assert sc[(ALPHA, 50)] <= 0.85 * sc[(0.0, 200)]
    assert sc[(ALPHA, 32)] <= 1.1 * sc[(0.0, 200)]


def test_trace_with_momentum(capsys):
    """verbose prints the momentum run's per-iteration rms waveform change.  Bound: the parity bound of
    test_parity_400_point_path for this input and iteration count (3x the reference's float32 / float64
    waveform distance), or 3x the distance of the two reference traces if that is larger.  The device sums
    its squares in float32 over 7,920 samples and ~120 atomics; the reference's float32 sum is pairwise, so
    the waveform distance is the one that covers the device's reduction."""
    amp = _amp_of_speech(8000, 11)
    ph = vo.initial_phase(amp.shape, 3)
    n = 8
    t64, t32 = [], []
    w64 = fr.griffin_lim_momentum(amp, 400, 80, n, ALPHA, phase0=ph, trace=t64)
    w32 = fr.griffin_lim_momentum(amp, 400, 80, n, ALPHA, phase0=ph, trace=t32, dtype=np.float32)
    got = _device(amp, 400, 80, n, ALPHA, ph, verbose=True)
    lines = [l for l in capsys.readouterr().out.splitlines() if 'mrse_delta' in l]
    assert len(lines) == n - 1
    vals = np.array([float(l.split('=')[-1]) for l in lines])
    bound = 3.0 * max(fr.rel_l2(w32, w64), fr.rel_l2(t32, t64))
    assert 0.0 < bound and fr.rel_l2(vals, t64) <= bound, (fr.rel_l2(vals, t64), bound)
    # the traced run computes the same waveform as the untraced one
    assert np.array_equal(got, _device(amp, 400, 80, n, ALPHA, ph))


def test_from_power_to_wav_batch_with_momentum():
    """The batched driver (power -> amplitude -> fast GL -> inverse pre-emphasis) at the bench's
    settings on a short batch: finite, normalised, and the momentum run is not the plain one."""
    import audio_lib
    from conftest import FE_KW
    y = fo.synth_speech(2, 12000, seed=3)
    _, _, P = audio_lib.calc_MFCC_input_batch(torch.from_numpy(y).cuda(), None, **FE_KW)
    ph = torch.from_numpy(np.random.RandomState(1).uniform(0, np.pi, tuple(P.shape)).astype(np.float32))
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80, win_length=400, mean_abs_amp_norm=0.045,
              n_iter=32, n_fft=None, realse=1.0, phase0=ph)
    w0 = audio_lib.from_power_to_wav_batch(P, None, **kw).cpu().numpy()
    w1 = audio_lib.from_power_to_wav_batch(P, None, momentum=ALPHA, **kw).cpu().numpy()
    assert np.isfinite(w1).all() and np.allclose(np.abs(w1).mean(1), 0.045, rtol=1e-4)
    assert not np.array_equal(w0, w1)
