"""Inputs of the general noise-gain check (tests/test_denoise_cpu.py, tests/test_denoise_gpu.py): a launch is (n_bins, rule,
frame counts, noise0 given or not) on a batch of four power spectrograms -- two of a noisy synthetic vowel under the
transform that has n_bins bins, two of exponentially distributed noise (the periodogram of Gaussian noise) at a level that
changes from bin to bin.  The bins put a wave's seams at 64 / 65 and at 192 / 201; the frame counts sit around n_init = 8
and hold 0, one long utterance and a count above max_frames."""
import functools

import numpy as np

import denoise_ref as dr
import vocoder_kernels_ref as vr

NBINS = (9, 33, 64, 65, 201, 257)
N_INIT = 8
# name: (max_frames, frame counts as the device gets them; utterances 0, 1: vowel, 2, 3: noise)
LAUNCHES = {'long': (300, (300, 0, 70, 400)), 'short': (N_INIT + 1, (1, N_INIT - 1, N_INIT, N_INIT + 1))}
SEED = 3                 # tests/test_denoise_cpu.py holds these inputs to at most 5 % of lanes near the 0.99 guard
HOP = 80


@functools.lru_cache(maxsize=None)
def _vowels():
    out = []
    for hz, seed in ((120.0, SEED), (210.0, SEED + 1)):
        clean, noise = dr.noisy_vowel(hz, 10.0, seed, seconds=2.1, lead=0.3)
        out.append(clean + noise)
    return out


@functools.lru_cache(maxsize=None)
def inputs(nb, kind):
    """(P float32 [4, max_frames, nb], counts, noise0 float32 [4, nb])."""
    maxF, counts = LAUNCHES[kind]
    n_fft = 2 * (nb - 1)
    w = vr.device_window(vr.padded_window(n_fft, n_fft))
    rng = np.random.RandomState(SEED + 100 * nb + len(kind))
    P = np.zeros((4, maxF, nb), np.float32)
    for b, x in enumerate(_vowels()):
        P[b] = (np.abs(vr.stft_wave(x, w, HOP)[:maxF]) ** 2).astype(np.float32)
    level = 10.0 ** rng.uniform(-4.0, 0.0, (2, 1, nb))
    P[2:] = (level * rng.exponential(1.0, (2, maxF, nb))).astype(np.float32)
    noise0 = (P[:, :N_INIT].mean(axis=1) * rng.uniform(0.5, 2.0, (4, nb))).astype(np.float32)
    P.setflags(write=False)
    noise0.setflags(write=False)
    return P, counts, noise0


@functools.lru_cache(maxsize=None)
def reference(nb, rule, kind, with_noise0):
    """(gain64, noise64, left_out [4, max_frames, nb] bool, bound_gain, bound_noise): the float64 run on the float32 inputs,
    the elements a lane leaves out from the frame on at which its float64 pb comes within 1e-5 of the 0.99 guard, and the
    bounds -- 4 x the float32 twin's own largest distance from float64 over the elements kept, absolute for the gain (it
    lives in [gain_min, 1]) and relative for the noise power (its level spans four decades across the bins).  The factor 4: the device's
    exp and log and numpy's differ by a few ulp each, and the recursion contracts."""
    P, counts, noise0 = inputs(nb, kind)
    cfg = dr.config(rule=rule, n_init=N_INIT)
    n0 = noise0 if with_noise0 else None
    g64, s64, pb = dr.noise_gain(P, counts, n0, cfg, trace=True)
    g32, s32 = dr.noise_gain(P, counts, n0, cfg, dtype=np.float32)
    out = dr.guard_mask(pb)
    keep = ~out
    live = keep & (s64 > 0.0)                                       # a written row: s >= FLT_MIN
    return (g64, s64, out, 4.0 * float(np.abs(g32 - g64)[keep].max()), 4.0 * float((np.abs(s32 - s64)[live] / s64[live]).max()))


def lanes_left_out(left_out, counts):
    """The share of the live lanes (utterance, bin) of which any frame is left out."""
    live = np.array([min(max(c, 0), left_out.shape[1]) > 0 for c in counts])
    return float(left_out.any(axis=1)[live].mean())
