"""Configurations and inputs of the general front-end tests (test_frontend_general_cpu.py / _gpu.py).

Every configuration is here for a code path of csrc/vc_frontend.hip (column `reaches`), every input is small.  A
configuration is the keyword dictionary of audio_lib.calc_MFCC_input."""
import functools

import numpy as np

from conftest import FE_KW
from oracle import frontend_oracle as fo
import frontend_general_ref as ref


def _kw(**over):
    kw = dict(FE_KW)
    kw.update(over)
    return kw


# id -> (configuration at its listed flags, kernel routing, launches above 64 KB of dynamic LDS, what it reaches)
CASES = {
    'ref-defaults': (_kw(hop_length=40, n_mels=128, n_mfcc=40, calc_mfcc_derivate=False), 'power400', (),
                     'power400<0> aliased, finalize<0,0,0>'),
    'hop160': (_kw(hop_length=160), 'power400', (), 'power400<80>, finalize<80,40,201>'),
    'sr22050': (_kw(sr=22050), 'power400', (), 'power400<80>, finalize<80,40,201> at hop 80 (widest filter 16)'),
    'sr8000': (_kw(sr=8000), 'fast400', (), 'the shipped path with another mel table'),
    'wide-mel': (_kw(n_mels=260, n_mfcc=13), 'power400', (), 'lds_alias == 0, empty filters'),
    'big-finalize-80': (_kw(n_mels=128, n_mfcc=80), 'power400', ('finalize',), 'finalize above 64 KB'),
    'big-finalize-128': (_kw(n_mels=128, n_mfcc=128), 'power400', ('finalize',), 'finalize above 64 KB, n_mfcc == n_mels'),
    'big-power400': (_kw(hop_length=560), 'power400', ('power',), 'power400 above 64 KB, fe_abssum'),
    'tiny': (_kw(n_fft=64, win_length=48, hop_length=16, n_mels=10, n_mfcc=10), 'generic', (),
             'generic, NM % 4 == 2, n_mfcc == n_mels, padded window'),
    'tiny-empty': (_kw(n_fft=64, win_length=64, hop_length=16, n_mels=40, n_mfcc=13, calc_mfcc_derivate=False), 'generic', (),
                   'generic, empty filters, odd cepstra'),
    'abssum': (_kw(n_fft=256, win_length=256, hop_length=160, n_mels=30, n_mfcc=7, window='hamming', calc_mfcc_derivate=False),
               'generic', (), 'fe_abssum, !fused_abs'),
    'gap': (_kw(n_fft=128, win_length=128, hop_length=200, n_mels=13, n_mfcc=13, calc_mfcc_derivate=False), 'generic', (),
            'hop > n_fft, fe_abssum'),
    'one-cep': (_kw(n_fft=1024, win_length=800, hop_length=256, n_mels=128, n_mfcc=1), 'generic', (), 'n_mfcc == 1'),
    'max-fft': (_kw(n_fft=2048, win_length=2048, hop_length=512, n_mels=80, n_mfcc=40, calc_mfcc_derivate=False), 'generic',
                ('power',), 'generic above 64 KB'),
}
IDS = tuple(CASES)
NOT_FAST400 = tuple(i for i in IDS if CASES[i][1] != 'fast400')
ALL_FLAG_IDS = ('tiny', 'hop160', 'abssum')         # these run every flag set
ABSSUM_IDS = ('abssum', 'gap', 'big-power400')
OVER_64K = tuple(i for i in IDS if CASES[i][2])

# The structure of each mel table: id -> (non-zeros, widest filter, empty filters).
TABLE_FACTS = {
    'ref-defaults': (394, 9, 0), 'hop160': (391, 14, 0), 'sr22050': (390, 16, 0), 'sr8000': (392, 12, 0),
    'wide-mel': (396, 5, 47), 'big-finalize-80': (394, 9, 0), 'big-finalize-128': (394, 9, 0), 'big-power400': (391, 14, 0),
    'tiny': (54, 13, 0), 'tiny-empty': (60, 4, 7), 'abssum': (241, 23, 0), 'gap': (113, 22, 0), 'one-cep': (1009, 24, 0),
    'max-fft': (2004, 75, 0),
}

# Dynamic LDS of the launches above 64 KB: id -> {launch: bytes}.
LDS_FACTS = {'big-finalize-80': {'finalize': 71088}, 'big-finalize-128': {'finalize': 102960},
             'big-power400': {'power': 66752}, 'max-fft': {'power': 88692}}


def kw_of(cid):
    return dict(CASES[cid][0])


# ------------------------------------------------------------------------------------------ flag sets
def _flags(norm, pre, first, delta, clip, factor):
    return dict(mean_abs_amp_norm=norm, pre_emphasis=pre, mfcc_normaleze_first_mfcc=first, calc_mfcc_derivate=delta,
                clip_output=clip, mfcc_norm_factor=factor, M_dB_norm_factor=factor, P_dB_norm_factor=factor)


# every flag takes both of its values at least twice, and each of A / B is the other's opposite
FLAG_SETS = {
    'A': _flags(0.003, 0.97, True, True, True, 0.01),
    'B': _flags(1.0, 0.0, False, False, False, 1.0),
    'C': _flags(0.003, 0.0, True, False, False, 1.0),
    'D': _flags(1.0, 0.97, False, True, True, 0.01),
    'E': _flags(0.003, 0.97, False, True, False, 0.01),
    'F': _flags(1.0, 0.0, True, True, True, 1.0),
}


def opposite(kw):
    """The flag set with every flag at its other value."""
    return _flags(1.0 if kw['mean_abs_amp_norm'] != 1.0 else 0.003, 0.0 if kw['pre_emphasis'] != 0.0 else 0.97,
                  not kw['mfcc_normaleze_first_mfcc'], not kw['calc_mfcc_derivate'], not kw['clip_output'],
                  1.0 if kw['mfcc_norm_factor'] != 1.0 else 0.01)


def variants(cid):
    """[(name, configuration)]: all flag sets for ALL_FLAG_IDS, the listed flags plus their opposite for the others."""
    kw = kw_of(cid)
    if cid in ALL_FLAG_IDS:
        return [(n, dict(kw, **f)) for n, f in FLAG_SETS.items()]
    return [('listed', kw), ('opposite', dict(kw, **opposite(kw)))]


ALL_VARIANTS = tuple((cid, name) for cid in IDS for name, _ in variants(cid))


def variant_kw(cid, name):
    return dict(variants(cid))[name]


# ------------------------------------------------------------------------------------------ inputs
# Noise has rare deep spectral nulls; one that lands just above the top_db floor is where float32 has least headroom.  The
# seeds are ones for which every input passes test_float32_headroom_of_the_inputs (which pins them).
SEED_BASE = 3000


def frame_counts(kw):
    """Frame counts on the seams of the stage-2 tile (G) and of the 32-frame finalize tile; at most 20 frames on n_fft 2048
    (a direct DFT of 2 M multiply-adds per frame)."""
    G = ref.tile_frames(ref.n_fft_of(kw))
    want = [2, G - 1, G, G + 1, 2 * G + 1, 33, 65]
    if ref.n_fft_of(kw) == 2048:
        want = [f for f in want if f <= 20]
    return want


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(wav [B, Lmax] float32, zero beyond each utterance; lens [B]).  Utterance b has frame_counts()[b] frames -- or the
    fewest a length above n_fft/2 gives, where that is more -- and a remainder L % hop that differs from one to the next."""
    kw = kw_of(cid)
    n_fft, hop = ref.n_fft_of(kw), kw['hop_length']
    rng = np.random.RandomState(SEED_BASE + IDS.index(cid))
    lens = []
    for b, F in enumerate(frame_counts(kw)):
        r = (0, hop - 1, hop // 2, 1, hop // 3, 0, hop - 2)[b] % hop
        lens.append(max(hop * (F - 1) + r, n_fft // 2 + 1 + b))
    sig = []
    for b, L in enumerate(lens):
        kind = b % 7
        if kind in (1, 4, 6):
            # speech-like.  synth_speech's own noise lies 45 dB under its harmonics, and the deepest of some 30,000 noise
            # bins another 40 dB under that: at the top_db floor, where a float32 transform of 1,024 or 2,048 points has no
            # headroom left (test_float32_headroom_of_the_inputs).  More noise lifts those bins by 20 dB.
            x = fo.synth_speech(1, L, seed=50 + b, sr=kw['sr'])[0].astype(np.float64) + 0.125 * rng.standard_normal(L)
        if kind in (1, 6):                              # two levels
            x *= 0.3 if kind == 1 else 2.0
        elif kind == 4:                                 # digital silence inside
            run = n_fft + 2 * hop
            s = max(1, (L - run) // 2)
            x[s:s + run] = 0.0
        else:                                           # white noise at four gains
            x = rng.standard_normal(L) * {0: 0.3, 2: 1e-3, 3: 0.01, 5: 3e-6}[kind]
            if kind == 3:
                x[L - 1] = 1.0                          # full-scale click in the last frame
        sig.append(x.astype(np.float32))
    wav = np.zeros((len(lens), max(lens)), np.float32)
    for b, x in enumerate(sig):
        assert np.abs(x).max() > 0
        wav[b, :len(x)] = x
    wav.setflags(write=False)
    return wav, tuple(lens)


# ------------------------------------------------------------------------------------------ tolerances
DB_TOL = {'mfcc': 1e-2, 'mel': 1e-2, 'pow': 2e-2}        # dB; an output scaled by a factor is held to factor x this


def tol(name, kw):
    factor = {'mfcc': kw['mfcc_norm_factor'], 'mel': kw['M_dB_norm_factor'], 'pow': kw['P_dB_norm_factor']}[name]
    return DB_TOL[name] * factor


# ------------------------------------------------------------------------------------------ hand-written stage-3 data
EXACT_IDS = ('tiny', 'hop160', 'abssum')
EXACT_SETS = ('range120', 'range30', 'below_amin', 'late_max', 'nan_padding')
EXACT_FACTOR = 1.0 / 128


def exact_kw(cid, norm=1.0):
    return dict(kw_of(cid), **_flags(norm, 0.97, True, True, True, EXACT_FACTOR))


def exact_lens(cid):
    """Four utterances; the third is one frame longer than the second has tiles for (see 'late_max')."""
    kw = kw_of(cid)
    G = ref.tile_frames(ref.n_fft_of(kw))
    return tuple(kw['hop_length'] * (F - 1) + 3 for F in (2 * G + 1, G + 1, 2 * G + 1, 65))


@functools.lru_cache(maxsize=None)
def exact_data(cid, name):
    """Raw dB arrays on a 1/8 dB grid, per utterance: [(pow_raw [F, NB], mel_raw [F, NM])], float64.  With factors of 1/128
    and mean_abs_amp_norm = 1 every intermediate of the power and mel outputs is a float32 number."""
    kw = kw_of(cid)
    n_fft, hop = ref.n_fft_of(kw), kw['hop_length']
    G = ref.tile_frames(n_fft)
    rng = np.random.RandomState(7 + EXACT_IDS.index(cid) * 10 + EXACT_SETS.index(name))
    out = []
    for b, L in enumerate(exact_lens(cid)):
        F = ref.num_frames(L, hop)
        shapes = ((F, 1 + n_fft // 2), (F, kw['n_mels']))
        if name == 'range120':          # the floor binds; the minimum after the floor is the floor
            lo, hi = -90.0, 30.0
        elif name == 'below_amin':      # every value under -100 dB: the amin clamp binds, all outputs 0
            lo, hi = -250.0, -101.0
        else:                           # 30 dB: the minimum is the true minimum and maps to exactly 0
            lo, hi = -20.0 - 3.0 * b, 10.0 - 3.0 * b
        arrs = [np.round(rng.uniform(lo, hi, s) * 8.0) / 8.0 for s in shapes]
        for a in arrs:                  # the extremes are taken, each once, away from frame 0
            a[F // 2, 1], a[F - 1, 0] = hi, lo
        if name == 'late_max':
            # utterances 1 and 2 share their first G + 1 frames; 2 goes on, and its maximum sits in its last tile, in a frame
            # 1 does not have, 81 dB above the maximum of 1: the floor of 2 lies above everything it shares with 1
            if b == 2:
                for a, prev in zip(arrs, out[1]):
                    a[:G + 1] = prev
                    a[2 * G, 2] = prev.max() + 81.0
        out.append(tuple(arrs))
    return tuple(out)
