"""Numpy restatement of the two noise-suppression launches (include/vc_hip.h, "Noise suppression"): vc_stft_power_f32 and
vc_noise_gain_f32.  float64 by default; with dtype=np.float32 the gain is a TWIN of the kernel: the same operations in the
same order, each rounded once (numpy never contracts a product into a sum), so that the configurations without a
transcendental come out bit for bit and the others differ by the few ulp between numpy's exp / log and the device's.
The STFT is tests/vocoder_kernels_ref.py's; the synthetic vowel is tests/diff_ref.py's resonator cascade."""
import math

import numpy as np

import vocoder_kernels_ref as vr

FLT_MIN = float(np.finfo(np.float32).tiny)
U = 2.0 ** -24
E1_SMALL = (-0.57721566, 0.99999193, -0.24991055, 0.05519968, -0.00976004, 0.00107857)      # Abramowitz & Stegun 5.1.53
E1_NUM = (8.5733287401, 18.0590169730, 8.6347608925, 0.2677737343)                          # 5.1.56
E1_DEN = (9.5733223454, 25.6329561486, 21.0996530827, 3.9584969228)
DEFAULTS = dict(rule=1, n_init=8, a_dd=0.98, xi_h1=10.0 ** 1.5, xi_min=10.0 ** -2.5, gain_min=0.1, gamma_max=1000.0)


def smoothing(hop, sr, tau_spp_ms=151.9, tau_noise_ms=71.7):
    hop_ms = 1000.0 * float(hop) / float(sr)
    return math.exp(-hop_ms / tau_spp_ms), math.exp(-hop_ms / tau_noise_ms)


def config(**kw):
    """A full configuration: DEFAULTS, the smoothing constants of the shipped hop (80 samples at 16 kHz), then ``kw``."""
    a_spp, a_noise = smoothing(80, 16000)
    c = dict(DEFAULTS, a_spp=a_spp, a_noise=a_noise)
    c.update(kw)
    return c


def e1(x, dtype=np.float64):
    """E1(x), x > 0, in the kernel's Horner form."""
    T = dtype
    x = np.asarray(x, T)
    with np.errstate(all='ignore'):
        xs = np.minimum(x, T(1.0))
        q = T(E1_SMALL[5])
        for a in E1_SMALL[4::-1]:
            q = q * xs + T(a)
        small = q - np.log(xs)
        xl = np.maximum(x, T(1.0))
        n, d = xl + T(E1_NUM[0]), xl + T(E1_DEN[0])
        for a, b in zip(E1_NUM[1:], E1_DEN[1:]):
            n, d = n * xl + T(a), d * xl + T(b)
        large = (np.exp(-xl) / xl) * (n / d)
    return np.where(x <= T(1.0), small, large).astype(T)


def noise_gain(P, n_frames=None, noise0=None, cfg=None, dtype=np.float64, trace=False):
    """P [B, maxF, nb] -> (gain, noise) [B, maxF, nb] of ``dtype``, rows at or beyond the clamped frame count 0.  cfg: a dict
    with the fields of vc_denoise_cfg (``config``).  With trace: (gain, noise, pb [B, maxF, nb]) -- the smoothed
    speech-presence probability the 0.99 guard reads.  One loop over the frames, all utterances and bins at once; an
    utterance past its last frame is carried along and its rows stay 0."""
    T = dtype
    c = config() if cfg is None else cfg
    P = np.asarray(P, T)
    B, maxF, nb = P.shape
    F = np.full(B, maxF) if n_frames is None else np.clip(np.asarray(n_frames, np.int64), 0, maxF)
    gain, noise, pbs = np.zeros((B, maxF, nb), T), np.zeros((B, maxF, nb), T), np.zeros((B, maxF, nb), T)
    one, half = T(1.0), T(0.5)
    a_spp, a_noise, a_dd = T(c['a_spp']), T(c['a_noise']), T(c['a_dd'])
    xi_h1, xi_min, gain_min, gamma_max = T(c['xi_h1']), T(c['xi_min']), T(c['gain_min']), T(c['gamma_max'])
    k1 = one + xi_h1
    c1 = xi_h1 / k1
    q_spp, q_n, q_dd = one - a_spp, one - a_noise, one - a_dd
    tiny, guard, v_min = T(FLT_MIN), T(np.float32(0.99)), T(np.float32(1e-6))
    with np.errstate(all='ignore'):
        if noise0 is not None:
            s = np.array(noise0, T)
        else:
            n0 = np.minimum(int(c['n_init']), F)
            acc = np.zeros((B, nb), T)
            for f in range(int(n0.max()) if B else 0):
                acc = np.where((f < n0)[:, None], acc + P[:, f], acc)
            s = acc / np.maximum(n0, 1).astype(T)[:, None]
        s = np.maximum(s, tiny)
        pb = np.full((B, nb), 0.5, T)
        A = np.zeros((B, nb), T)
        for f in range(int(F.max()) if B else 0):
            y = P[:, f]
            t = np.minimum((y / s) * c1, T(80.0))
            p = one / (one + k1 * np.exp(-t))
            pb = a_spp * pb + q_spp * p
            p = np.where(pb > guard, np.minimum(p, guard), p)
            e = (one - p) * y + p * s
            s = np.maximum(a_noise * s + q_n * e, tiny)
            g = np.minimum(y / s, gamma_max)
            r = np.ones((B, nb), T) if f == 0 else np.minimum(A / s, gamma_max)
            xi = np.maximum(a_dd * r + q_dd * np.maximum(g - one, T(0.0)), xi_min)
            w = xi / (one + xi)
            G = w
            if int(c['rule']) == 1:
                G = w * np.exp(half * e1(np.maximum(w * g, v_min), T))
            G = np.minimum(np.maximum(G, gain_min), one)
            A = (G * G) * y
            live = (f < F)[:, None]
            gain[:, f], noise[:, f], pbs[:, f] = np.where(live, G, 0), np.where(live, s, 0), np.where(live, pb, 0)
    return (gain, noise, pbs) if trace else (gain, noise)


def guard_mask(pb, n_frames=None, margin=1e-5):
    """[B, maxF, nb] bool: True from the first frame on at which a lane's float64 pb comes within ``margin`` of 0.99 -- the one
    discontinuity of the recursion, where a rounding error may send the two runs different ways."""
    near = np.abs(np.asarray(pb, np.float64) - 0.99) <= margin
    return np.cumsum(near, axis=1) > 0


# ------------------------------------------------------------------------------------------ power
def frames_of(length, n_frames, max_frames, n_fft, hop):
    """F_b of vc_stft_filter_f32 / vc_stft_power_f32."""
    F = min(max_frames, 1 + length // hop)
    if n_frames is not None:
        F = min(F, max(int(n_frames), 0))
    return 0 if (length <= n_fft // 2 or hop * (F - 1) <= n_fft // 2) else F


def power(x, length, n_frames, max_frames, w, hop):
    """(P [max_frames, nb] float64, F_b, bound [max_frames, nb]) of one utterance x[0, length): |stft|^2 and the float32
    model's bound on it.  Either component of a bin is a float32 sum whose longest chain is vr.chain_of(n_fft) additions,
    so it is off by at most e = (chain + 8) u sum_n |w[n] x[n]| (vr.forward_bound without its overlap-add term: the
    waveform is read as it is); then |re'^2 + im'^2 - re^2 - im^2| <= 2 (|re| + |im|) e + 2 e^2, plus three roundings of
    the squares and their sum."""
    N = len(w)
    nb = 1 + N // 2
    F = frames_of(length, n_frames, max_frames, N, hop)
    P, bound = np.zeros((max_frames, nb)), np.zeros((max_frames, nb))
    if F:
        xs = np.asarray(x[:length], np.float64)
        fr = vr._framed(xs, N, hop)[:F]
        Z = np.fft.rfft(fr * w, axis=1)
        e = ((vr.chain_of(N) + 8) * U * (np.abs(fr) * np.abs(w)).sum(axis=1))[:, None]
        re, im = np.abs(Z.real), np.abs(Z.imag)
        P[:F] = re * re + im * im
        bound[:F] = 2.0 * (re + im) * e + 2.0 * e * e + 3.0 * U * ((re + e) ** 2 + (im + e) ** 2)
    return P, F, bound


# ------------------------------------------------------------------------------------------ the synthetic recording
def noisy_vowel(f0_hz, snr_db, seed, seconds=1.5, lead=0.6, sr=16000, vib=0.03, vib_hz=5.0):
    """(clean, noise) float64 [n]: ``lead`` seconds of silence, then a three-formant /a/ (tests/diff_ref.py) on a pulse train
    with +-vib vibrato; white noise at ``snr_db`` below the vowel's own mean power (measured over the vowel, not the lead)."""
    import diff_ref
    n, n0 = int(seconds * sr), int(lead * sr)
    t = np.arange(n - n0) / float(sr)
    f0 = f0_hz * (1.0 + vib * np.sin(2.0 * np.pi * vib_hz * t))
    clean = np.zeros(n)
    clean[n0:] = diff_ref.vowel(diff_ref.pulse_train(f0, sr), *diff_ref.VOWEL_A, sr=sr)
    clean[n0:n0 + 160] *= np.linspace(0.0, 1.0, 160)                 # a 10 ms onset, not a click
    sigma = np.sqrt((clean[n0:] ** 2).mean() / 10.0 ** (snr_db / 10.0))
    return clean, sigma * np.random.RandomState(seed).standard_normal(n)


def istft_filter(x, G, w, hop):
    """y = istft(G * stft(x)) over the frames of G, float64: hop (F - 1) samples."""
    Z = vr.stft_wave(np.asarray(x, np.float64), w, hop)[:len(G)]
    return vr.waveform(vr.frames_from_spectrum(Z * G, w), w, hop)


def _db(v):
    return 10.0 * np.log10(v)


def snr_figures(clean, noise, gain, w, hop, lead_samples, y=None):
    """(input SNR, output SNR) in dB over the vowel, away from its onset and from the last window.  The output is
    ``y`` (default: the float64 filter under ``gain`` [F, nb]); its error is everything that is not the vowel as the
    unit-gain transform pair returns it, attenuated or distorted speech included."""
    gain = np.asarray(gain, np.float64)
    L = hop * (len(gain) - 1)
    if y is None:
        y = istft_filter(clean + noise, gain, w, hop)
    y = np.asarray(y, np.float64)[:L]
    ref = istft_filter(clean, np.ones_like(gain), w, hop)
    a, b = lead_samples + len(w), L - len(w)
    return (float(_db((clean[a:b] ** 2).sum() / (noise[a:b] ** 2).sum())),
            float(_db((ref[a:b] ** 2).sum() / ((y[a:b] - ref[a:b]) ** 2).sum())))


def true_psd(noise, w):
    """The mean of a white noise's periodogram under the window w: sigma^2 sum w^2, the same in every bin."""
    return float(np.var(noise) * (w * w).sum())


def psd_error_db(noise_est, n_frames, psd):
    """The tracker's last estimate [nb] against the true noise power, in dB, median over the bins."""
    return float(np.median(_db(np.asarray(noise_est, np.float64)[n_frames - 1] / psd)))


def lead_figures(P, gain, noise_est, psd, lead_frames, cfg):
    """(attenuation, expected attenuation, bias) in dB over the SECOND HALF of the noise-only lead (frames lead/2 ..
    lead - 5: the tracker has had four of its time constants, and no window touches the vowel).
    attenuation = sum P / sum G^2 P there.  A rule that sat on its floor would give floor_db exactly; two things keep it
    above.  The periodogram of noise is exponentially distributed, and the frames in its tail get a gain above the floor
    even when the noise level is known; and the tracker underestimates the level by ``bias`` = median over those frames and
    all bins of noise_est / psd, which moves every frame up that tail.  ``expected`` holds both: the attenuation of the
    same rule on the same P with the noise level FROZEN (a_noise = 1) at psd * bias."""
    P, gain, noise_est = (np.asarray(v, np.float64) for v in (P, gain, noise_est))
    fr = slice(lead_frames // 2, lead_frames - 5)
    att = _db(P[fr].sum() / (gain[fr] ** 2 * P[fr]).sum())
    bias = float(np.median(_db(noise_est[fr] / psd)))
    frozen = np.full((1, P.shape[1]), psd * 10.0 ** (bias / 10.0))
    g0, _ = noise_gain(P[None], None, frozen, dict(cfg, a_noise=1.0))
    return float(att), float(_db(P[fr].sum() / (g0[0, fr] ** 2 * P[fr]).sum())), bias
