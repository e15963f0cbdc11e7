"""Configurations and inputs of the vocoder kernel tests (tests/test_vocoder_kernels_cpu.py, tests/test_vocoder_kernels_gpu.py).

A case is (n_fft, win_length, hop, window, frame counts of a ragged batch).  The batch holds the smallest utterance the
reflect padding admits (hop (F - 1) > n_fft / 2), one workgroup's tile of frames plus one frame (the next multiple of the
tile above that minimum where one tile is too short), an utterance with a partial last tile that sets max_frames, and an
utterance whose magnitudes are all zero.  At most 70 frames, at most 10 at n_fft >= 2048.

Magnitudes are those of synthetic speech under the case's own transform (the speech played at the speed that fits the
transform's length, see inputs()) plus a floor of FLOOR of the peak, so no bin of a valid row is zero outside the all-zero
utterance; the initial phase is drawn once, in [0, pi), from a fixed seed.  tests/test_vocoder_kernels_cpu.py holds these
inputs to what the device tests need of them: every bound a share under 1e-3 of what it guards, every 400-point case under
the cap of the plain late-iteration check."""
import functools

import numpy as np

from oracle.frontend_oracle import synth_speech
import vocoder_kernels_ref as ref


def _hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _hamming(n):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _skew(n):
    """Asymmetric: periodic Hann times a rising ramp (positive from tap 1 on)."""
    return _hann(n) * (0.5 + np.arange(n) / n)


# name: (n_fft, win_length, hop, window taps builder or None for the plan's own periodic Hann, frames of the utterances;
#        the LAST utterance is the all-zero one)
CASES = {
    'ship':          (400, 400, 80, None, (4, 17, 37, 23)),
    'hop40':         (400, 400, 40, None, (7, 17, 41, 20)),
    'hop81':         (400, 400, 81, None, (4, 17, 35, 9)),
    'hop100-win320': (400, 320, 100, None, (4, 17, 22, 6)),
    'hop200':        (400, 400, 200, None, (3, 17, 19, 5)),
    'hop400':        (400, 400, 400, None, (2, 17, 21, 5)),
    'hop7':          (400, 400, 7, None, (30, 33, 70, 31)),
    'hamming':       (400, 400, 80, _hamming, (4, 17, 34, 18)),
    'skew':          (400, 400, 80, _skew, (4, 17, 39, 16)),
    'rect-hop400':   (400, 400, 400, np.ones, (2, 17, 18, 3)),
    'n2':            (2, 2, 1, None, (3, 5, 11, 6)),
    'n16':           (16, 12, 5, None, (3, 5, 14, 7)),
    'n64-hop64':     (64, 64, 64, None, (2, 5, 11, 6)),
    'n512':          (512, 400, 128, None, (4, 5, 14, 7)),
    'n800':          (800, 800, 40, None, (12, 13, 22, 14)),
    'n2048':         (2048, 2048, 512, None, (4, 5, 10, 6)),
    'n4096':         (4096, 4096, 1024, None, (4, 5, 10, 7)),
    'skew16':        (16, 16, 4, _skew, (4, 5, 15, 6)),
}
ALL = tuple(CASES)
POINT400 = tuple(c for c in ALL if CASES[c][0] == 400)
GENERIC = tuple(c for c in ALL if CASES[c][0] != 400)
# the cases whose plain late-iteration model stays under ref.PLAIN_CAP (tests/test_vocoder_kernels_cpu.py pins this list)
IN_CAP = POINT400 + ('n2', 'n16', 'n64-hop64', 'skew16')
SEED = 8                 # tests/test_vocoder_kernels_cpu.py holds the inputs to what the checks need of them: every 400-point case under the cap
# (n_fft + 8) 2^-24 is 2.4e-4 at 4,096 points, so a bound under 1e-3 of the peak needs sum |t_i| under four times the peak
# after the overlap-add; the synthetic speech's noise alone is a third of that.  From 2,048 points on, bins under GATE of the
# utterance's peak therefore carry the floor alone.
GATE_FROM, GATE = 2048, 0.1
FLOOR = 1e-3             # of the utterance's peak at up to 201 bins; above, the floor's sum over the bins stays what it is there


def geometry(cid):
    n_fft, win, hop, _, frames = CASES[cid]
    return n_fft, win, hop, frames


def taps(cid):
    """float64 [win_length] for h_window, or None where the plan builds its own periodic Hann."""
    _, win, _, make, _ = CASES[cid]
    return None if make is None else np.ascontiguousarray(make(win), dtype=np.float64)


def window(cid):
    """The padded window as the device holds it (rounded to float32), float64 [n_fft]."""
    n_fft, win, _, _, _ = CASES[cid]
    return ref.device_window(ref.padded_window(win, n_fft, taps(cid)))


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(amp [B, max_frames, bins] float32, phase0 the same) of the ragged batch; rows at or beyond an utterance's frame
    count hold NaN; the last utterance's valid rows are zero."""
    n_fft, win, hop, frames = geometry(cid)
    w, nb, B, maxF = window(cid), ref.num_bins(n_fft), len(frames), max(frames)
    rng = np.random.RandomState(SEED + len(cid))
    amp = np.full((B, maxF, nb), np.nan, np.float32)
    ph = np.full((B, maxF, nb), np.nan, np.float32)
    for b, F in enumerate(frames):
        L = hop * (F - 1)
        # played at the speed at which a frame of n_fft samples holds what a frame of 400 holds at 16 kHz (linear
        # interpolation): a few pitch periods at every size, and the synthetic speech's own white noise, which alone would
        # put sum |t_i| of a 4,096-point transform at eight times its peak, stays in the band it has at 400 points
        speed = 400.0 / n_fft
        src = synth_speech(1, int(np.ceil(L * speed)) + 2, seed=SEED + 10 * b)[0].astype(np.float64)
        y = np.interp(np.arange(L) * speed, np.arange(len(src)), src)
        a = np.abs(ref.stft_wave(y, w, hop))
        assert a.shape == (F, nb)
        if n_fft >= GATE_FROM:
            a = np.where(a >= GATE * a.max(), a, 0.0)
        amp[b, :F] = a + FLOOR * min(1.0, 201.0 / nb) * a.max() * rng.rand(F, nb)
        ph[b, :F] = rng.uniform(0.0, np.pi, (F, nb))
    amp[B - 1, :frames[-1]] = 0.0
    amp.setflags(write=False)
    ph.setflags(write=False)
    return amp, ph


def single(cid, b):
    """(amp [F, bins], phase0 [F, bins]) float64 of utterance b."""
    F = geometry(cid)[3][b]
    amp, ph = inputs(cid)
    return amp[b, :F].astype(np.float64), ph[b, :F].astype(np.float64)
