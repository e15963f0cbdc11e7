"""Host reference of the speech-activity masks (include/vc_hip.h, "Speech activity"), numpy.

  frames      F = 1 + len // hop, the front-end's and the tracker's count
  energy      e[f] = sum_{j < W} x[s + j]^2, s = f * hop - W // 2, zeros outside [0, len)
  raw         'energy': e > 0 and e > r * max e, r = float32(10^(-top_db / 10));  'voiced': f0 > 0;  'energy+voiced': both
  smoothing   every run of inactive frames of length <= max_gap with an active frame on both sides becomes active; then
              every run of active frames shorter than min_run becomes inactive (runs at either end: their own length)
  compaction  index = the active frames ascending, n_active their count, n_kept = n_active, or F (index = 0 .. F-1) when
              none is active; a second mask is ANDed in first over the frames i < min(F_a, F_b)
  intervals   the maximal runs of active frames as [start, end), none when no frame is active

``frame_energy(..., dtype=np.float64)`` is the definition.  ``dtype=np.float32`` is the restatement in the device's
order of operations: 64 partial sums, partial l a chain of fused multiply-adds over the samples l, l + 64, ... of the
frame (a float64 product of two float32 values is exact, so rounding acc + x * x once from float64 restates the fused
operation), then the butterfly: every partial adds partial l ^ 32, then l ^ 16, ... l ^ 1.

``speech_gain`` is the gain the masked waveform-level scores hand to the front-end in place of its own normalisation over
the whole waveform.  ``masked_pipeline`` is the float64 pipeline of a masked score: mcd_ref.dtw on the compacted cepstra, the path mapped back
to original frame numbers, f0_ref.metrics along it.
"""
import numpy as np

import f0_ref
import mcd_ref

MARGIN = 1e-4               # |e / (r * max) - 1| below this: the float32 decision may fall either way
MODES = ('energy', 'voiced', 'energy+voiced')


def n_frames(length, hop):
    return 1 + int(length) // int(hop)


def frames(x, hop, W):
    """[F, W] matrix of the frames, zeros outside the signal."""
    x = np.asarray(x)
    F = n_frames(len(x), hop)
    idx = (np.arange(F) * hop - W // 2)[:, None] + np.arange(W)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    src = x if len(x) else np.zeros(1, x.dtype)                       # an empty utterance: one frame of zeros
    return np.where(ok, src[np.clip(idx, 0, len(src) - 1)], 0).astype(x.dtype)


def frame_energy(x, hop=80, W=400, dtype=np.float64):
    fr = frames(np.asarray(x, dtype=np.float32), hop, W)               # the samples are float32 on either side
    if dtype != np.float32:
        return (fr.astype(np.float64) ** 2).sum(axis=1)
    F = fr.shape[0]
    n = -(-W // 64) * 64
    pad = np.zeros((F, n), np.float64)                                  # a lane past the frame's end adds nothing
    pad[:, :W] = fr
    pad = pad.reshape(F, n // 64, 64)
    v = np.zeros((F, 64), np.float32)
    for k in range(n // 64):
        live = (k * 64 + np.arange(64)) < W
        v = np.where(live[None, :], (v.astype(np.float64) + pad[:, k, :] ** 2).astype(np.float32), v)      # fmaf(x, x, v)
    lanes = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ s]).astype(np.float32)
    return v[:, 0]


def ratio(top_db):
    return np.float32(10.0 ** (-float(top_db) / 10.0))


def raw_energy(e, top_db=40.0):
    """(decision [F] bool, marginal [F] bool) of float64 energies."""
    e = np.asarray(e, dtype=np.float64)
    thr = float(ratio(top_db)) * (e.max() if len(e) else 0.0)
    raw = (e > 0) & (e > thr)
    with np.errstate(divide='ignore', invalid='ignore'):
        marginal = np.abs(e / thr - 1.0) < MARGIN if thr > 0 else np.zeros(len(e), bool)
    return raw, marginal


def runs(mask):
    """[(value, start, end)] of the maximal runs of a 0 / 1 sequence."""
    m = np.asarray(mask).astype(bool)
    out, s = [], 0
    for f in range(1, len(m) + 1):
        if f == len(m) or m[f] != m[s]:
            out.append((bool(m[s]), s, f))
            s = f
    return out if len(m) else []


def smooth(mask, max_gap=20, min_run=0):
    m = np.asarray(mask).astype(bool).copy()
    F = len(m)
    for v, s, e in runs(m):                                             # 1. short gaps between two active frames
        if not v and s > 0 and e < F and e - s <= max_gap:
            m[s:e] = True
    for v, s, e in runs(m):                                             # 2. short active runs, whatever they touch
        if v and e - s < min_run:
            m[s:e] = False
    return m


def intervals(mask):
    return np.array([(s, e) for v, s, e in runs(mask) if v], dtype=np.int64).reshape(-1, 2)


def compact(mask_a, mask_b=None):
    """dict(index [n_kept], n_active, n_kept, intervals [n, 2]) of one utterance; mask_b is ANDed in over the common frames."""
    m = np.asarray(mask_a).astype(bool)
    if mask_b is not None:
        F = min(len(m), len(mask_b))
        m = m[:F] & np.asarray(mask_b).astype(bool)[:F]
    idx = np.nonzero(m)[0].astype(np.int64)
    n_active = len(idx)
    if n_active == 0:
        idx = np.arange(len(m), dtype=np.int64)
    return dict(index=idx, n_active=n_active, n_kept=len(idx), intervals=intervals(m) if n_active else np.zeros((0, 2), np.int64))


def path_map(path, index_a, index_b):
    p = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    return np.stack([np.asarray(index_a)[p[:, 0]], np.asarray(index_b)[p[:, 1]]], axis=1)


def activity(x, hop=80, W=400, mode='energy', top_db=40.0, max_gap=20, min_run=0, f0=None, energy=None):
    """The float64 mask of one utterance: dict(raw, marginal, mask, energy) + compact(mask).  ``energy``: energies to decide
    on in place of the float64 ones (the device's own); ``f0``: the track of the voiced modes (f0_ref.yin by default)."""
    assert mode in MODES
    e = frame_energy(x, hop, W) if energy is None else np.asarray(energy, np.float64)
    raw, marginal = np.ones(len(e), bool), np.zeros(len(e), bool)
    if mode != 'voiced':
        raw, marginal = raw_energy(e, top_db)
    if mode != 'energy':
        if f0 is None:
            f0 = f0_ref.yin(x, hop=hop)[0]
        raw = raw & (np.asarray(f0)[:len(e)] > 0)
    mask = smooth(raw, max_gap, min_run)
    out = dict(raw=raw, marginal=marginal, mask=mask, energy=e)
    out.update(compact(mask))
    return out


def masked_pipeline(ca, cb, mask_a, mask_b, f0_a, f0_b, scale=1.0, band=None, dtype=np.float64):
    """DTW over the kept frames of float64 cepstra ca [Fa, C], cb [Fb, C], the path in original frame numbers, the F0
    figures along it on the original tracks.  Returns dict(total, path_len, mcd, path, n_active_a, n_active_b, metrics)."""
    a, b = compact(mask_a), compact(mask_b)
    total, n, p = mcd_ref.dtw(np.asarray(ca)[a['index']], np.asarray(cb)[b['index']], scale, band, dtype)
    path = path_map(p, a['index'], b['index'])
    return dict(total=total, path_len=n, mcd=total / n, path=path, n_active_a=a['n_active'], n_active_b=b['n_active'],
                metrics=f0_ref.metrics(f0_a, f0_b, len(mask_a), len(mask_b), path))


def speech_gain(x, mask, hop=80, target=0.003):
    """target / mean |x| over the samples of the active frames: sample i belongs to frame min((i + hop // 2) // hop, F - 1);
    over all samples when no frame is active; 1 when they are all zero.  float64."""
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(mask).astype(bool)
    act = m[np.minimum((np.arange(len(x)) + hop // 2) // hop, len(m) - 1)] if m.any() else np.ones(len(x), bool)
    s = np.abs(x[act]).sum()
    return float(target) * act.sum() / s if s > 0 else 1.0


def noise_floor(n, peak, rng, db=-60.0):
    """White noise `db` below a peak: what a recording's "silence" is (not zeros, so the front-end's floor is exercised)."""
    return (peak * 10.0 ** (db / 20.0) * rng.standard_normal(n)).astype(np.float32)


def broadband_utterance(seed, seconds=2.0, sr=16000):
    """A speech-like signal whose mel cells sit above the front-end's floor: 30 harmonics (amplitudes 1 / h) of a gliding
    fundamental plus white noise a tenth of the peak, under one slow amplitude modulation that never reaches zero."""
    rng = np.random.RandomState(seed)
    n = int(seconds * sr)
    t = np.arange(n) / float(sr)
    f0 = rng.uniform(100.0, 200.0) * 2.0 ** (0.3 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t))
    env = 1.0 + 0.5 * np.sin(2 * np.pi * rng.uniform(2.0, 5.0) * t)
    x = env * (0.2 * f0_ref.harmonic_tone(f0, sr, n_harm=30) + 0.05 * rng.standard_normal(n))
    return x.astype(np.float32)


def silence_pair(seed=31, sr=16000, lead=0.5, pause=0.3, trail=2.0, cut=0.95):
    """(a, b, edits): broadband_utterance(seed) over a noise floor 60 dB below its peak, and the same samples with `lead`
    seconds of that floor in front, a `pause` cut in at `cut` seconds and `trail` seconds behind.
    Every piece is a whole number of hops (80), so a frame of b away from an edit reads the samples its frame of a reads.
    edits: the four sample positions in b where speech and floor meet."""
    rng = np.random.RandomState(seed)
    s = broadband_utterance(seed)
    peak = float(np.abs(s).max())
    a = (s + noise_floor(len(s), peak, rng)).astype(np.float32)
    n_lead, n_pause, n_trail, c = int(lead * sr), int(pause * sr), int(trail * sr), int(cut * sr)
    b = np.concatenate([noise_floor(n_lead, peak, rng), a[:c], noise_floor(n_pause, peak, rng), a[c:], noise_floor(n_trail, peak, rng)])
    return a, b.astype(np.float32), (n_lead, n_lead + c, n_lead + c + n_pause, n_lead + n_pause + len(a))
