"""Shapes and inputs of the dereverberation tests (tests/test_dereverb_cpu.py, tests/test_dereverb_gpu.py): the smallest at
which each path of vc_wpe_f32 can go wrong, not the workload's own.

A solver case is (batch, n_bins, max_frames, n_frames or None, K, D, I, c, floor_rel, load_rel).  Between them:
  frames    0, D, D + 1, D + K - 1, D + K, 17 and 33 (either side of the transform's tile of 16), the documented cap
            vc_wpe_max_frames(32), max_frames that is no multiple of 16, and counts ragged within a batch, a 0 among them
  taps      1, 2, 4, 16, 32          delay  1, 5, 64          iterations  1, 3
  context   0, 2 -- with the clamped edges t < c and t >= F - c in every case that has c > 0
  bins      2, 3, 201, 257 (n_fft = 512: the generic transform's count)
and the special bins of special_bins().  The spectra are complex Gaussian noise run through a two-tap recursion along time,
so that there is something to predict; seeded per case."""
import numpy as np

import dereverb_ref as ref

FLOOR, LOAD = 1e-6, 1e-8
#                 B  bins  maxF  n_frames                      K   D   I  c  floor  load
CASES = {
    'edges-k4':  (7, 3,    35,   (0, 5, 6, 8, 9, 17, 33),      4,  5,  3, 2, FLOOR, LOAD),     # F = 0, D, D+1, D+K-1, D+K, 17, 33
    'ragged3':   (3, 2,    37,   (37, 0, 20),                  2,  1,  1, 0, FLOOR, LOAD),
    'k1-d64':    (1, 2,    100,  None,                         1,  64, 3, 2, FLOOR, LOAD),
    'k16-ship':  (2, 201,  61,   (61, 40),                     16, 5,  3, 1, FLOOR, LOAD),
    'k32-n257':  (1, 257,  90,   None,                         32, 5,  1, 0, 1e-3,  0.0),
    'cap-k32':   (1, 2,    ref.max_frames(32), None,           32, 5,  1, 2, FLOOR, LOAD),
}
ALL = tuple(CASES)


def cfg_of(cid):
    _, _, _, _, K, D, I, c, floor, load = CASES[cid]
    return dict(taps=K, delay=D, iterations=I, context=c, floor_rel=floor, load_rel=load)


def spectra(cid, seed=None, poison=True):
    """(re, im float32 [B, bins, maxF], n_frames or None).  Frames at or beyond an utterance's count hold NaN: nothing may
    read them (poison=False: they hold spectrum like the others, for a caller that moves the counts about)."""
    B, nb, maxF, nf = CASES[cid][:4]
    rng = np.random.RandomState(sum(map(ord, cid)) if seed is None else seed)
    z = rng.standard_normal((B, nb, maxF)) + 1j * rng.standard_normal((B, nb, maxF))
    for t in range(2, maxF):
        z[:, :, t] += 0.6 * z[:, :, t - 1] - 0.3j * z[:, :, t - 2]
    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
    if nf is not None and poison:
        for b, n in enumerate(nf):
            re[b, :, n:], im[b, :, n:] = np.nan, np.nan
    return re, im, (None if nf is None else list(nf))


SPECIAL_F, SPECIAL_K, SPECIAL_D = 40, 4, 2


def special_bins():
    """(re, im float32 [1, 5, 40]) for K = 4, D = 2:
      bin 0  all zero: m == 0, the first pivot is 0 / 0, status 1
      bin 1  constant 1 + 0.5i from frame 0 on
      bin 2  noise (an ordinary bin between the special ones)
      bin 3  one impulse at frame F - D - 2: its history reaches taps 0 and 1 only, so R = diag(r, r, 0, 0) -- singular, and
             solved only because of the load; with load = 0 the third pivot is 0: status 1, passthrough
      bin 4  the constant again, negated
    About the constant bin: it is NOT rank 1 under the header's definition.  The frames t < D + K - 1 see a partial history
    (c, 0, 0, 0), (c, c, 0, 0), ... and those vectors are independent, so R is positive definite with or without the load
    (tests/test_dereverb_cpu.py pins what the restatement gives for it); bin 3 is the singular one."""
    F = SPECIAL_F
    rng = np.random.RandomState(77)
    z = np.zeros((1, 5, F), np.complex128)
    z[0, 1] = 1.0 + 0.5j
    z[0, 2] = rng.standard_normal(F) + 1j * rng.standard_normal(F)
    z[0, 3, F - SPECIAL_D - 2] = 0.75 - 0.25j
    z[0, 4] = -1.0 - 0.5j
    return z.real.astype(np.float32), z.imag.astype(np.float32)
