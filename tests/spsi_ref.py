"""CPU reference of the deterministic Griffin-Lim phase start (include/vc_hip.h vc_phase_spsi): single-pass spectrogram
inversion (Beauregard, Harish & Wyse 2015) in the exact fixed-point form the device computes.

Phase is an unsigned 32-bit fraction of a turn; addition wraps mod 2^32 = one turn.  Per frame, from its magnitudes
m (float32) alone:
    peak   k in 1 .. nb-2 with m[k] > m[k-1] and m[k] > m[k+1] (strict float32 comparisons)
    owner  a peak owns itself; a non-peak bin b in 1 .. nb-2 is owned by the peak k > b with m[j] < m[j+1] for all
           b <= j < k, else by the peak k < b with m[j] < m[j-1] for all k < j <= b (a valley both sides reach goes to
           the higher-frequency peak); bins 0, nb-1 and bins no peak reaches are unowned
    inc(k) = uint32(((hop*k) % n_fft << 32) // n_fft) + uint32(rint(float64(p) * (hop * 2^32 / n_fft))),
           p = 0.5f * (a - d) / ((a - 2.0f*c) + d) in float32 with (a, c, d) = m[k-1], m[k], m[k+1]; a p that is not
           finite or exceeds 1 in magnitude (only infinite or negative magnitudes produce one) counts as 0
    v(t, b) = v(t-1, k) + inc(k) + (((b - k) & 1) << 31) for an owned bin, v(t-1, b) otherwise, v(-1, .) = 0
    phase  = float32(int32(v)) * float32(pi / 2^31)

phase_sequential is that loop; phase_chunked composes the per-frame maps b -> (owner, offset) over chunks and scans the
chunks (the device's three launches); phase_float64 is the textbook form with float accumulation in radians.

Not a test module (no test_ prefix): tests/test_spsi_cpu.py and tests/test_spsi_gpu.py import it.
"""
import numpy as np

from fgla_ref import vo                 # the oracle's STFT, as tests/fgla_ref.py takes it

PI_SCALE = np.float32(np.pi / 2.0 ** 31)


def owners(m):
    """m [nb] float32 -> int64 [nb]: the owning peak of every bin, -1 for an unowned one."""
    m = np.asarray(m, dtype=np.float32)
    nb = m.shape[0]
    idx = np.arange(nb)
    own = np.full(nb, -1, dtype=np.int64)
    if nb < 3:
        return own
    with np.errstate(invalid='ignore'):
        up = np.zeros(nb, bool)
        up[:-1] = m[:-1] < m[1:]                                   # up[j]: m[j] < m[j+1]
        down = np.zeros(nb, bool)
        down[1:] = m[1:] < m[:-1]                                  # down[j]: m[j] < m[j-1]
        peak = np.zeros(nb, bool)
        peak[1:-1] = (m[1:-1] > m[:-2]) & (m[1:-1] > m[2:])
    ku = np.minimum.accumulate(np.where(up, nb, idx)[::-1])[::-1]   # end of the rising run that starts at b
    kd = np.maximum.accumulate(np.where(down, -1, idx))             # start of the falling run that ends at b
    up_ok = (ku > idx) & peak[np.minimum(ku, nb - 1)]
    down_ok = (kd < idx) & peak[np.maximum(kd, 0)]
    own = np.where(peak, idx, np.where(up_ok, ku, np.where(down_ok, kd, -1)))
    own[0] = own[-1] = -1
    return own.astype(np.int64)


def owners_literal(m):
    """The definition word for word, O(nb^2): the check of owners()."""
    m = np.asarray(m, dtype=np.float32)
    nb = m.shape[0]
    with np.errstate(invalid='ignore'):
        peaks = [k for k in range(1, nb - 1) if m[k] > m[k - 1] and m[k] > m[k + 1]]
        own = np.full(nb, -1, dtype=np.int64)
        for b in range(1, nb - 1):
            if b in peaks:
                own[b] = b
                continue
            hi = [k for k in peaks if k > b and all(m[j] < m[j + 1] for j in range(b, k))]
            lo = [k for k in peaks if k < b and all(m[j] < m[j - 1] for j in range(k + 1, b + 1))]
            if hi:
                own[b] = hi[0]
            elif lo:
                own[b] = lo[-1]
    return own


def peak_offset(m, n_fft, hop):
    """p [nb] float32 (0 where it does not count) for every bin taken as a peak centre."""
    m = np.asarray(m, dtype=np.float32)
    p = np.zeros(m.shape[0], dtype=np.float32)
    a, c, d = m[:-2], m[1:-1], m[2:]
    with np.errstate(all='ignore'):
        q = (np.float32(0.5) * (a - d)) / ((a - np.float32(2.0) * c) + d)
        q = np.where(np.abs(q) <= np.float32(1.0), q, np.float32(0.0)).astype(np.float32)
    p[1:-1] = q
    return p


def increments(m, n_fft, hop):
    """inc [nb] uint32 for every bin taken as a peak centre."""
    nb = np.asarray(m).shape[0]
    k = np.arange(nb, dtype=np.uint64)
    whole = (((np.uint64(hop) * k) % np.uint64(n_fft)) << np.uint64(32)) // np.uint64(n_fft)
    scale = float(hop) * 4294967296.0 / float(n_fft)
    frac = np.rint(peak_offset(m, n_fft, hop).astype(np.float64) * scale).astype(np.int64)
    return ((whole.astype(np.int64) + frac) & 0xFFFFFFFF).astype(np.uint32)


def frame_map(m, n_fft, hop):
    """One frame's map: v(t, b) = v(t-1, src[b]) + off[b].  Returns (src int64 [nb], off uint32 [nb])."""
    nb = np.asarray(m).shape[0]
    idx = np.arange(nb)
    own = owners(m)
    inc = increments(m, n_fft, hop)
    owned = own >= 0
    k = np.where(owned, own, idx)
    half = (((idx - k) & 1).astype(np.uint32) << np.uint32(31))
    off = np.where(owned, inc[k] + half, np.uint32(0)).astype(np.uint32)      # uint32 addition wraps
    return k, off


def to_phase(v):
    return v.astype(np.int32).astype(np.float32) * PI_SCALE


def _frames(amp, n_frames):
    amp = np.asarray(amp, dtype=np.float32)
    F = amp.shape[0] if n_frames is None else int(n_frames)
    return amp, F


def phase_sequential(amp, n_fft, hop, n_frames=None, return_state=False):
    """amp [Fmax, nb] float32 -> phase [Fmax, nb] float32 (0 beyond n_frames): the recurrence frame by frame."""
    amp, F = _frames(amp, n_frames)
    Fmax, nb = amp.shape
    v = np.zeros(nb, dtype=np.uint32)
    out = np.zeros((Fmax, nb), dtype=np.float32)
    state = np.zeros((Fmax, nb), dtype=np.uint32)
    for t in range(F):
        src, off = frame_map(amp[t], n_fft, hop)
        v = v[src] + off
        state[t] = v
        out[t] = to_phase(v)
    return (out, state) if return_state else out


def phase_chunked(amp, n_fft, hop, chunk, n_frames=None):
    """The same through the device's three steps: per chunk of `chunk` frames compose the frame maps from the identity
    (src'[b] = src[q[b]], off'[b] = off[q[b]] + w[b]), scan the chunk maps from V[0] = 0, replay each chunk from V[c]."""
    amp, F = _frames(amp, n_frames)
    Fmax, nb = amp.shape
    chunk = int(chunk)
    starts = list(range(0, F, chunk))
    maps = []
    for t0 in starts:                                              # 1: one map per chunk
        src, off = np.arange(nb), np.zeros(nb, dtype=np.uint32)
        for t in range(t0, min(t0 + chunk, F)):
            q, w = frame_map(amp[t], n_fft, hop)
            src, off = src[q], off[q] + w
        maps.append((src, off))
    V = [np.zeros(nb, dtype=np.uint32)]                            # 2: the state at every chunk's start
    for src, off in maps[:-1]:
        V.append(V[-1][src] + off)
    out = np.zeros((Fmax, nb), dtype=np.float32)
    for c, t0 in enumerate(starts):                                # 3: replay
        v = V[c]
        for t in range(t0, min(t0 + chunk, F)):
            q, w = frame_map(amp[t], n_fft, hop)
            v = v[q] + w
            out[t] = to_phase(v)
    return out


def phase_float64(amp, n_fft, hop, n_frames=None):
    """Textbook SPSI in float64 radians: phase advance 2 pi hop (k + p) / n_fft per peak, accumulated in floating point,
    neighbours locked to their peak with a half turn on every odd one.  The peaks, the owners and the float32 peak offset
    p are the definition's, so the two forms differ in the accumulation alone."""
    amp, F = _frames(amp, n_frames)
    Fmax, nb = amp.shape
    v = np.zeros(nb, dtype=np.float64)
    out = np.zeros((Fmax, nb), dtype=np.float64)
    idx = np.arange(nb)
    for t in range(F):
        own = owners(amp[t])
        p = peak_offset(amp[t], n_fft, hop).astype(np.float64)
        owned = own >= 0
        k = np.where(owned, own, idx)
        adv = 2.0 * np.pi * hop * (k + p[k]) / n_fft + np.pi * ((idx - k) & 1)
        v = np.where(owned, v[k] + adv, v)
        out[t] = v
    return out


def wrapped_distance(a, b):
    """max |a - b| mod 2 pi, radians (float64)."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.max(np.abs((d + np.pi) % (2.0 * np.pi) - np.pi))) if d.size else 0.0


def voiced_signal(n_samples, seed=0, sr=16000):
    """The synthetic voiced signal: f0 = 120 + 40 sin(2 pi 1.3 t), harmonics 1..29 of weight
    exp(-0.5 ((h f0 - 700) / 900)^2 + 0.1) / h, amplitude (0.5 + 0.5 sin(2 pi 3 t))^2, 0.01 white noise, pre-emphasis 0.97."""
    t = np.arange(int(n_samples)) / float(sr)
    f0 = 120.0 + 40.0 * np.sin(2.0 * np.pi * 1.3 * t)
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    y = np.zeros_like(t)
    for h in range(1, 30):
        y += np.exp(-0.5 * ((h * f0 - 700.0) / 900.0) ** 2 + 0.1) / h * np.sin(h * ph)
    y *= (0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * t)) ** 2
    y += 0.01 * np.random.RandomState(seed).standard_normal(len(t))
    return np.append(y[0], y[1:] - 0.97 * y[:-1])


def voiced_magnitudes(n_frames, n_fft=400, hop=80, seed=0):
    """|STFT| of the voiced signal, [bins, n_frames] float64 (the oracle's layout; .T.astype(float32) is the device's)."""
    y = voiced_signal(hop * (int(n_frames) - 1), seed)
    return np.abs(vo.stft(y, n_fft, hop, n_fft)).astype(np.float64)
