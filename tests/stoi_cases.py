"""The named inputs of tests/test_stoi_cpu.py and tests/test_stoi_gpu.py.  Everything is float32-representable (the device
and the float64 restatement read the same numbers) and deterministic.  tests/test_stoi_cpu.py asserts, in float64, that no
frame energy of any case lies within a relative 1e-3 of its keep threshold, so the device's kept list must be exact."""
import numpy as np

import stoi_ref as sr

H, W = sr.H, sr.W
QUIET = 1e-5            # "silence" that is not digital: 100 dB below the speech-like stretches


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def len_for_frames(K):
    """The shortest length with exactly K frames (K >= 1)."""
    return W + H * (K - 1) + 1


def noise(n, seed, amp=0.1):
    return _f32(amp * np.random.RandomState(seed).standard_normal(n))


def gaps(seed=3):
    """6,000 samples: a quiet lead of 1,000, speech-like noise, a quiet interior gap of 1,500 (the gather crosses
    non-adjacent frames), speech-like noise, a quiet tail of 700."""
    x = noise(6000, seed)
    q = noise(6000, seed + 1, QUIET)
    for a, b in ((0, 1000), (2600, 4100), (5300, 6000)):
        x[a:b] = q[a:b]
    return _f32(x)


def modulated(n, seed):
    """Noise under a slow envelope that stays within 20 dB: every frame is kept, no two segments are alike."""
    t = np.arange(n) / float(sr.FS)
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + seed)
    return _f32(noise(n, seed) * env)


def energy_batch():
    """(wav [B, Lmax] float64 with NaN from each length on, lens): L in {0, 256, 257, 384, 385, 4000}, an utterance of
    digital silence, and ``gaps``."""
    lens = [0, 256, 257, 384, 385, 4000, 4000, 6000]
    Lmax = 6005
    wav = np.full((len(lens), Lmax), np.nan)
    for b, n in enumerate(lens):
        wav[b, :n] = noise(n, 10 + b)
    wav[6, :4000] = 0.0
    wav[7, :6000] = gaps()
    return wav, lens


def impulse():
    """(x, p, amplitude): one impulse at sample p = 5 H + 40, inside frames 4 (offset 168) and 5 (offset 40) alone."""
    x = np.zeros(len_for_frames(9))
    x[5 * H + 40] = 0.75
    return x, 5 * H + 40, 0.75


def cosine(k0=40, K=4):
    """A cosine centred on bin k0 of the 512-point transform; K frames, all kept."""
    n = np.arange(len_for_frames(K))
    return _f32(0.3 * np.cos(2.0 * np.pi * k0 * n / sr.NFFT + 0.4))


BAND_CASES = ('K1', 'K2', 'K3', 'K5', 'K16', 'K17', 'K18', 'K31', 'impulse', 'cosine', 'gaps')


def band_case(name):
    """(x, y) float64 of one length; the processed signal is the reference plus noise at about 5 dB."""
    if name.startswith('K'):
        x = noise(len_for_frames(int(name[1:])), 40 + int(name[1:]))
    elif name == 'impulse':
        x = impulse()[0]
    elif name == 'cosine':
        x = cosine()
    else:
        x = gaps()
    return x, _f32(x + noise(len(x), 77, 0.056))


SCORE_K = (30, 31, 32, 38, 39)          # M = 29, 30, 31 (S = 0, 1, 2) and M = 37, 38 (S = 8, 9: the seam of the 8-segment tile)


def score_batch():
    """(ref [B, Lmax], deg [B, Lmax], lens): modulated noise of exactly K frames, K over SCORE_K, and the same plus noise at
    about 5 dB; NaN from each length on."""
    lens = [len_for_frames(K) for K in SCORE_K]
    Lmax = max(lens) + 3
    ref, deg = np.full((len(lens), Lmax), np.nan), np.full((len(lens), Lmax), np.nan)
    for b, n in enumerate(lens):
        ref[b, :n] = modulated(n, 60 + b)
        deg[b, :n] = _f32(ref[b, :n] + noise(n, 90 + b, 0.04))
    return ref, deg, lens


SI_SDR_LENS = (0, 1, 1023, 1024, 1025)


def si_sdr_batch():
    """(ref, deg, lens, tags): the lengths around 1,024 lanes, a reference of zeros, deg == ref, and a pair on a DC offset
    of 100 times its amplitude; NaN from each length on."""
    lens = list(SI_SDR_LENS) + [700, 700, 3000, 700, 4]
    tags = ['len%d' % n for n in SI_SDR_LENS] + ['x=0', 'y=x', 'dc', 'y=0', 'orthogonal']
    Lmax = 3004
    ref, deg = np.full((len(lens), Lmax), np.nan), np.full((len(lens), Lmax), np.nan)
    for b, n in enumerate(lens):
        ref[b, :n] = noise(n, 120 + b)
        deg[b, :n] = _f32(ref[b, :n] + noise(n, 140 + b, 0.03))
    ref[5, :700] = 0.0
    deg[6, :700] = ref[6, :700]
    ref[7, :3000] = _f32(ref[7, :3000] + 10.0)
    deg[7, :3000] = _f32(deg[7, :3000] + 9.0)
    deg[8, :700] = 0.0
    ref[9, :4], deg[9, :4] = [1.0, -1.0, 1.0, -1.0], [0.5, 0.5, -0.5, -0.5]     # zero means, <x, y> == 0 exactly
    return ref, deg, lens, tags


def vowel_pair(snr_db):
    """(clean, noisy) float64: the modulated vowel and the vowel in white noise at snr_db."""
    x = _f32(sr.modulated_vowel())
    return x, _f32(x + sr.white_noise_at(x, snr_db, 7))


def every_reference():
    """(name, x, L) of every reference waveform a GPU case keeps frames of."""
    out = []
    wav, lens = energy_batch()
    out += [('energy%d' % b, np.nan_to_num(wav[b]), n) for b, n in enumerate(lens)]
    out += [('band-' + c, band_case(c)[0], len(band_case(c)[0])) for c in BAND_CASES]
    ref, _, lens = score_batch()
    out += [('score%d' % b, np.nan_to_num(ref[b]), n) for b, n in enumerate(lens)]
    out += [('vowel', vowel_pair(0)[0], len(vowel_pair(0)[0]))]
    return out
