"""CPU reference of fast Griffin-Lim (include/vc_hip.h vc_griffin_lim_momentum_f32): the loop of
oracle.vocoder_oracle.griffin_lim_alg (audio_lib.py:249-274) with librosa's momentum term.

With beta = momentum / (1 + momentum) and R_0 = 0, for i = 1 .. num_iters - 1:
    R_i = STFT(ISTFT(S_{i-1})),  C_i = R_i - beta R_{i-1},  S_i = amp * C_i / |C_i|
and wav = ISTFT(S_{num_iters-1}).  The first projection uses R_1 unchanged, so num_iters <= 2 does not
depend on the momentum, and momentum 0 is vocoder_oracle.griffin_lim_alg operation for operation.

dtype=np.float64 runs the oracle's istft / stft (its STFT stores complex64 like librosa.stft).
dtype=np.float32 runs the same transforms in single precision (numpy's float32 FFTs, float32 window,
overlap-add and normalisation) and keeps every quantity between steps in float32 / complex64
(waveform, R, C, S, beta): the distance between the two modes is the yardstick for the device's own
float32 error.

Not a test module (no test_ prefix): tests/test_vocoder_momentum_cpu.py and tests/test_vocoder_momentum_gpu.py
import it.
"""
import numpy as np

from oracle import frontend_oracle as fo
from oracle import vocoder_oracle as vo


def _istft32(spec, hop_length, win_length):
    """vocoder_oracle.istft in float32 arithmetic."""
    n_fft = 2 * (spec.shape[0] - 1)
    w = fo.fft_window('hann', win_length, n_fft).astype(np.float32)
    frames = np.fft.irfft(spec.astype(np.complex64), n=n_fft, axis=0) * w[:, None]   # [n_fft, F] float32
    n_frames = spec.shape[1]
    y = np.zeros(n_fft + hop_length * (n_frames - 1), dtype=np.float32)
    for i in range(n_frames):
        y[i * hop_length:i * hop_length + n_fft] += frames[:, i]
    wss = vo.window_sumsquare('hann', n_frames, hop_length, win_length, n_fft).astype(np.float32)
    nz = wss > vo.F32_TINY
    y[nz] /= wss[nz]
    return y[n_fft // 2:-(n_fft // 2)]


def _stft32(y, n_fft, hop_length, win_length):
    """vocoder_oracle.stft (frontend_oracle.stft) in float32 arithmetic."""
    w = fo.fft_window('hann', win_length, n_fft).astype(np.float32).reshape(-1, 1)
    yp = np.pad(np.asarray(y, np.float32), int(n_fft // 2), mode='reflect')
    n_frames = 1 + (len(yp) - n_fft) // hop_length
    idx = np.arange(n_fft)[:, None] + hop_length * np.arange(n_frames)[None, :]
    return np.fft.rfft(w * yp[idx], axis=0).astype(np.complex64)


def griffin_lim_momentum(stft_amp, win_length, hop_length, num_iters, momentum=0.0, n_fft=None, phase0=None,
                         seed=0, trace=None, dtype=np.float64):
    """stft_amp [1+n_fft/2, F] -> wav [hop*(F-1)] (dtype).  ``trace``: optional list that receives the rms
    difference between successive waveforms, like vocoder_oracle.griffin_lim_alg (computed in dtype)."""
    if n_fft is None:
        n_fft = win_length
    f32 = np.dtype(dtype) == np.float32
    cdt = np.complex64 if f32 else np.complex128
    stft_amp = np.asarray(stft_amp, dtype=dtype)
    if phase0 is None:
        phase0 = vo.initial_phase(stft_amp.shape, seed)
    beta = dtype(momentum / (1.0 + momentum))
    spec = stft_amp * np.exp(1j * np.asarray(phase0, dtype=dtype))
    if f32:
        spec = spec.astype(cdt)
    wav = last = rebuilt = None
    for i in range(num_iters):
        wav = _istft32(spec, hop_length, win_length) if f32 else vo.istft(spec, hop_length, win_length)
        if trace is not None and last is not None:
            d = last - wav                                      # float32 mode: a float32 reduction, like the device
            trace.append(float(np.sqrt(np.sum(d * d, dtype=dtype) / dtype(len(d)))))
        if i != num_iters - 1:
            if f32:
                d = _stft32(wav, n_fft, hop_length, win_length)
            else:
                d = vo.stft(wav, n_fft, hop_length, win_length).astype(cdt)
            c = d if rebuilt is None or momentum == 0.0 else (d - beta * rebuilt).astype(cdt)
            rebuilt = d
            spec = vo.project_phase(c, stft_amp)
            if f32:
                spec = spec.astype(cdt)
        last = wav
    return wav


def sc(wav, stft_amp, win_length, hop_length, n_fft=None):
    """Spectral convergence of a waveform (float64 evaluation)."""
    return vo.spectral_convergence(np.asarray(wav, np.float64), np.asarray(stft_amp, np.float64), win_length,
                                   hop_length, n_fft)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
