"""Host reference of differential-spectrum conversion (include/vc_hip.h, "Differential-spectrum conversion"; DESIGN.md
section 26): the gain of the filter in float64 and in the device's float32 order of operations, the filter itself
(y = istft(G * stft(x)) in librosa's sense) in float64, the float32 error bounds of both launches, and the synthetic vowels
and the spectral distance of the method's own check.  Plain numpy (scipy only for the vowels' resonators).

stft / istft are restated here on their own; tests/test_diff_cpu.py holds them against tests/vocoder_kernels_ref.py, whose
float32 model (u = 2^-24, a sum of n terms is off by at most (n + 8) u sum |t_i|) the bounds below are built from.  Nothing
here is fitted to a device result.
"""
import numpy as np

import vocoder_kernels_ref as vr

U = vr.U
LOG2_10_OVER_20 = np.float32(np.log2(10.0) / 20.0)        # the constant of the launch: power dB -> log2 of an amplitude ratio
EXP2_ULPS = 2                                           # exp2f: documented at 1 ulp; one more for the comparison's own rounding
MAX_TAPS = 65


# ------------------------------------------------------------------------------------------ the gain
def smoothing_taps(half_width):
    """conversion.diff_smoothing_taps restated: Hann shape over 2 h + 1 bins without zero end taps, float64, sum 1, float32."""
    h = int(half_width)
    c = 0.5 + 0.5 * np.cos(np.pi * np.arange(-h, h + 1, dtype=np.float64) / (h + 1))
    c = 0.5 * (c + c[::-1])
    return (c / c.sum()).astype(np.float32)


def refl(i, nb):
    """Mirror about bin 0 and about bin nb - 1 without repeating the edge, as often as it takes."""
    P = 2 * (nb - 1)
    m = np.mod(i, P)
    return np.where(m < nb, m, P - m)


def _valid(n_frames, b, F):
    return F if n_frames is None else min(max(int(n_frames[b]), 0), F)


def gain_s(pred, tru, n_frames, norm, taps, alpha, max_boost_db, max_cut_db, dtype=np.float64):
    """The clamped smoothed difference s [B, F, nb] in dB (rows at or beyond n_frames: NaN) in ``dtype``.  float64 is the
    definition on the float32 inputs and parameters; float32 is the launch's arithmetic: IEEE division, the sum ascending in
    j from +0 with every product and every sum rounded once, one product with alpha, the clamps."""
    pred, tru = np.asarray(pred, np.float32), np.asarray(tru, np.float32)
    B, F, nb = pred.shape
    c = np.asarray(taps, np.float32).astype(dtype)
    h = (len(c) - 1) // 2
    assert len(c) == 2 * h + 1 <= MAX_TAPS
    norm, alpha = dtype(np.float32(norm)), dtype(np.float32(alpha))
    lo, hi = dtype(-np.float32(max_cut_db)), dtype(np.float32(max_boost_db))
    s = np.full((B, F, nb), np.nan, dtype)
    k = np.arange(nb)
    for b in range(B):
        n = _valid(n_frames, b, F)
        d = (np.maximum(pred[b, :n], np.float32(0)).astype(dtype) - np.maximum(tru[b, :n], np.float32(0)).astype(dtype)) / norm
        acc = np.zeros((n, nb), dtype)
        for j in range(-h, h + 1):
            acc = acc + c[j + h] * d[:, refl(k + j, nb)]
        s[b, :n] = np.minimum(np.maximum(alpha * acc, lo), hi)
    return s


def gain_from_s(s):
    """G = 2 ** (s * float32(log2(10) / 20)), 0 where s is NaN (rows beyond n_frames).  A float32 s gives the launch's own
    float32 exponent, evaluated exactly (float64): what the device's exp2f is held against."""
    s = np.asarray(s)
    t = s * LOG2_10_OVER_20 if s.dtype == np.float32 else s * (np.log2(10.0) / 20.0)
    return np.where(np.isnan(s), 0.0, np.exp2(np.where(np.isnan(s), 0.0, t).astype(np.float64)))


def gain(pred, tru, n_frames, norm, taps, alpha=1.0, max_boost_db=20.0, max_cut_db=30.0, dtype=np.float64):
    return gain_from_s(gain_s(pred, tru, n_frames, norm, taps, alpha, max_boost_db, max_cut_db, dtype))


def exp2_rel_bound():
    """Relative bound of the device's exp2f on a given float32 exponent: EXP2_ULPS units in the last place, 2 u each."""
    return 2 * EXP2_ULPS * U


def gain_rel_bound(pred, tru, n_frames, norm, taps, alpha):
    """[B, F, nb]: relative bound on the device's G against the float64 definition, derived as
    vocoder_kernels_ref.power_to_amp_rel_bound: ln(10) / 20 times the absolute float32 error e of s, plus the exponential.
    d carries 2 u |d| (one subtraction, one division); the sum of n = n_taps products (n + 8) u sum |c_j d_j| by the model's
    rule (the 8 covers the products, d's own two roundings and the product with alpha); the clamps do not enlarge an error;
    the exponent s * float32(log2(10) / 20) carries 2 u |s| (the constant's rounding, the product's)."""
    pred, tru = np.asarray(pred, np.float32), np.asarray(tru, np.float32)
    B, F, nb = pred.shape
    c = np.abs(np.asarray(taps, np.float32).astype(np.float64))
    h = (len(c) - 1) // 2
    a = float(np.float32(alpha))
    out = np.zeros((B, F, nb))
    k = np.arange(nb)
    for b in range(B):
        n = _valid(n_frames, b, F)
        d = np.abs((np.maximum(pred[b, :n], 0).astype(np.float64) - np.maximum(tru[b, :n], 0).astype(np.float64)) / float(np.float32(norm)))
        t = np.zeros((n, nb))
        for j in range(-h, h + 1):
            t += c[j + h] * d[:, refl(k + j, nb)]
        e = a * (len(c) + 8) * U * t
        out[b, :n] = np.log(10.0) / 20.0 * (e + 2 * U * a * t) + exp2_rel_bound()
    return out


# ------------------------------------------------------------------------------------------ stft, istft, the filter
def padded(x, n_fft):
    """x reflect-padded by n_fft / 2 about sample 0 and about its last sample."""
    x = np.asarray(x, np.float64)
    half = n_fft // 2
    assert len(x) > half, 'shorter than the reflect padding'
    return np.concatenate([x[half:0:-1], x, x[-2:-half - 2:-1]])


def stft(x, w, hop, n_use=None):
    """[F, bins] complex128, F = 1 + len(x) // hop (the first n_use of them): frame f is the transform of
    w[n] * padded(x)[f hop + n]."""
    N = len(w)
    xp = padded(x, N)
    F = 1 + len(x) // hop if n_use is None else n_use
    S = np.empty((F, 1 + N // 2), np.complex128)
    for f in range(F):
        S[f] = np.fft.rfft(xp[f * hop:f * hop + N] * w)
    return S


def synthesis_frames(S, w):
    """w[n] * irfft(S_f)[n]  [F, n_fft]."""
    return np.fft.irfft(S, n=len(w), axis=1) * w


def istft_frames(fr, w, hop):
    """The frames overlap-added, divided by the window sum-square where that exceeds float32 tiny, trimmed by n_fft / 2:
    hop (F - 1) samples."""
    F, N = fr.shape
    y, wss = np.zeros(N + hop * (F - 1)), np.zeros(N + hop * (F - 1))
    for f in range(F):
        y[f * hop:f * hop + N] += fr[f]
        wss[f * hop:f * hop + N] += w * w
    ok = wss > vr.F32_TINY
    y[ok] /= wss[ok]
    return y[N // 2:N // 2 + hop * (F - 1)]


def istft(S, w, hop):
    return istft_frames(synthesis_frames(S, w), w, hop)


def frames_used(length, n_frames, max_frames, n_fft, hop):
    """F_b of the launch: the smallest of n_frames (None: absent), max_frames and 1 + len / hop, a negative count as 0; 0 for
    an utterance the reflect padding does not fit (len <= n_fft / 2 or hop (F - 1) <= n_fft / 2)."""
    F = min(max_frames, 1 + max(int(length), 0) // hop)
    if n_frames is not None:
        F = min(F, max(int(n_frames), 0))
    return 0 if (length <= n_fft // 2 or hop * (F - 1) <= n_fft // 2) else F


def stft_filter(x, G, w, hop, n_use=None):
    """y = istft(G[f] * stft(x)[f], f < F) float64 [hop (F - 1)], F = n_use or 1 + len(x) // hop; G [>= F, bins] real."""
    S = stft(x, w, hop, n_use)
    return istft(np.asarray(G, np.float64)[:len(S)] * S, w, hop)


def filter_bound(x, G, w, hop, n_use=None):
    """(y float64, bound [hop (F - 1)]) for the device's float32 pass on the float32 samples x and gains G with the window w as
    the device holds it.  By the model at the top of vocoder_kernels_ref.py:
      forward   either component of Z_f is a sum of chain terms: (chain + 8) u A_f, A_f = sum_n |w[n] xpad[f hop + n]|; the
                bin as a complex number moves by at most sqrt(2) of that; scaled by G
      product   G * Z rounds each component once: at most 2 u |G Z| on the bin
      ... both pushed through the inverse map (inverse_of_bound), plus the inverse half's own rounding on the spectrum it
      transforms (inverse_bound(G Z, w)); the total through the overlap-add (ola_of_bound), plus the overlap-add's own
      rounding, division included (ola_bound, on the reference frames), trimmed."""
    N = len(w)
    G = np.asarray(G, np.float64)
    S = stft(x, w, hop, n_use)
    F = len(S)
    xp = np.abs(padded(x, N))
    A = np.array([(xp[f * hop:f * hop + N] * np.abs(w)).sum() for f in range(F)])
    GZ = G[:F] * S
    dS = G[:F] * (np.sqrt(2.0) * (vr.chain_of(N) + 8) * U * A)[:, None] + 2 * U * np.abs(GZ)
    fr = synthesis_frames(GZ, w)
    fb = vr.inverse_of_bound(dS, w) + vr.inverse_bound(GZ, w)
    bound = vr.trim(vr.ola_of_bound(fb, w, hop) + vr.ola_bound(fr, w, hop), N)
    return istft_frames(fr, w, hop), bound


# ------------------------------------------------------------------------------------------ the method's own check
def frontend_power_db(x, w, hop, norm=0.01, mean_abs=0.003, pre_emphasis=0.97):
    """The front-end's normalised power dB [F, bins] (audio_lib.py:125-157, 230-240 restated in float64): level to a mean
    magnitude of mean_abs, pre-emphasis, |stft|^2 in dB with a floor at 1e-10 and 80 dB under the utterance's peak, the
    utterance's minimum removed, times norm, clipped to [-1, 1]."""
    x = np.asarray(x, np.float64)
    x = x * (mean_abs / np.abs(x).mean())
    x = np.concatenate([x[:1], x[1:] - pre_emphasis * x[:-1]])
    P = 10.0 * np.log10(np.maximum(1e-10, np.abs(stft(x, w, hop)) ** 2))
    P = np.maximum(P, P.max() - 80.0)
    return np.clip(norm * (P - P.min()), -1.0, 1.0)


def pulse_train(f0, sr=16000, top=7000.0):
    """Band-limited pulses of a fundamental given per sample: sum of cos(h phase) over the harmonics below ``top`` Hz."""
    f0 = np.asarray(f0, np.float64)
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(len(f0))
    for h in range(1, int(top / f0.min()) + 1):
        x += np.where(h * f0 < top, np.cos(h * ph), 0.0)
    return x


def vowel(excitation, formants, bandwidths, sr=16000):
    """The excitation through a cascade of two-pole resonators (one per formant), scaled to peak 0.5."""
    from scipy import signal
    y = np.asarray(excitation, np.float64)
    for fc, bw in zip(formants, bandwidths):
        r = np.exp(-np.pi * bw / sr)
        y = signal.lfilter([1.0 - r], [1.0, -2.0 * r * np.cos(2.0 * np.pi * fc / sr), r * r], y)
    return 0.5 * y / np.abs(y).max()


VOWEL_A = ((730.0, 1090.0, 2440.0), (90.0, 110.0, 170.0))       # Peterson & Barney's /a/ and /i/ (male averages)
VOWEL_I = ((270.0, 2290.0, 3010.0), (60.0, 100.0, 150.0))


def two_vowels(seconds=1.0, sr=16000, f_lo=70.0, f_hi=150.0):
    """(source, target, f0 per sample): the same pulse train, its fundamental gliding from f_lo to f_hi, through the
    formants of /a/ and of /i/."""
    n = int(seconds * sr)
    f0 = f_lo * (f_hi / f_lo) ** (np.arange(n) / float(n - 1))
    e = pulse_train(f0, sr)
    return vowel(e, *VOWEL_A, sr=sr), vowel(e, *VOWEL_I, sr=sr), f0


def smoothed_log_spectrum(x, w, hop, taps, sr=16000, top=4000.0):
    """10 log10 of the mean power spectrum over the frames, smoothed along frequency by ``taps`` (mirrored edges), the bins
    below ``top`` Hz, mean removed."""
    P = 10.0 * np.log10(np.maximum((np.abs(stft(x, w, hop)) ** 2).mean(axis=0), 1e-30))
    nb = len(P)
    c = np.asarray(taps, np.float64)
    h = (len(c) - 1) // 2
    k = np.arange(nb)
    s = sum(c[j + h] * P[refl(k + j, nb)] for j in range(-h, h + 1))
    s = s[:int(top / (sr / 2.0) * (nb - 1))]
    return s - s.mean()


def log_spectral_distance(a, b, w, hop, taps):
    """RMS difference in dB of the two signals' smoothed_log_spectrum."""
    d = smoothed_log_spectrum(a, w, hop, taps) - smoothed_log_spectrum(b, w, hop, taps)
    return float(np.sqrt((d * d).mean()))
