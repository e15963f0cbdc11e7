"""Restatement of pitch conversion (include/vc_hip.h, "Pitch") in numpy.

The plan is integer arithmetic throughout (python integers, so no width is assumed); the overlap-add is, per covering
grain, one rounded product and two rounded sums in the working dtype, and one division per sample.  The device is compared
against the float32 reading bit for bit.

  clamp_tables(period_q, ratio_q)          -> (P, S): the analysis and the synthesis step per frame, python integers
  marks(T, n, hop)                         the mark recurrence, mark by mark (the definition)
  marks_by_frame(T, n, hop)                the closed form: one ceiling division per frame
  plan(period_q, ratio_q, n, hop, M=None)  -> Plan(K, J, a, s, src, h [M] int32, -1 beyond)
  window()                                 W [2049] float32
  ola(x, n, p, w_floor, dtype)             -> (y [len(x)], D [len(x)]) in ``dtype``
  shift(x, n, period_q, ratio_q, hop, ...) plan + ola
  tables(f0, sr, ratio=, target_f0=, unvoiced_period=)   what conversion.pitch_tables computes, in numpy
  vowel(f0_per_sample, sr)                 harmonics of a fundamental under two formants
"""
from collections import namedtuple

import numpy as np

Q = 65536
P_MIN, P_MAX, S_MAX = 16 * Q, 1024 * Q, 2048 * Q
R_MIN, R_MAX = Q // 2, 2 * Q
WIN_N = 2048
Plan = namedtuple('psola_plan', 'K J a s src h')


def max_marks(max_len):
    return int(max_len) // 16 + 1


def clamp_tables(period_q, ratio_q):
    P = [min(max(int(v), P_MIN), P_MAX) for v in period_q]
    R = [min(max(int(v), R_MIN), R_MAX) for v in ratio_q]
    S = [min(max((p * Q + r // 2) // r, P_MIN), S_MAX) for p, r in zip(P, R)]
    return P, S


def frame_of(m, hop, F):
    return min((int(m) + hop // 2) // hop, F - 1)


def marks(T, n, hop):
    F, out, pos = len(T), [], 0
    while (pos >> 16) < n:
        out.append(pos >> 16)
        pos += T[frame_of(pos >> 16, hop, F)]
    return out


def marks_by_frame(T, n, hop):
    """Frame f holds the marks at pos + i * T[f] below its end ((f + 1) * hop - hop // 2) << 16 -- n << 16 for the last
    frame and for a frame that n cuts: ceil((end - pos) / T[f]) of them."""
    F, out, pos = len(T), [], 0
    for f in range(F):
        end = n << 16 if f == F - 1 else min(((f + 1) * hop - hop // 2) << 16, n << 16)
        if pos < end:
            c = -((pos - end) // T[f])
            out += [(pos + i * T[f]) >> 16 for i in range(c)]
            pos += c * T[f]
    return out


def nearest(a, v):
    """Index of the element of the ascending list ``a`` nearest to v, the lower of two equally near ones."""
    k = int(np.searchsorted(a, v, side='left'))
    if k >= len(a):
        return len(a) - 1
    if k > 0 and v - a[k - 1] <= a[k] - v:
        return k - 1
    return k


def plan(period_q, ratio_q, n, hop, M=None):
    n, hop = int(n), int(hop)
    M = max_marks(n) if M is None else int(M)
    P, S = clamp_tables(period_q, ratio_q)
    a, s = marks(P, n, hop), marks(S, n, hop)
    src = [a[nearest(a, v)] for v in s]
    h = [(P[frame_of(v, hop, len(P))] + 32768) >> 16 for v in src]
    pad = lambda v: np.array(list(v) + [-1] * (M - len(v)), dtype=np.int32)
    return Plan(len(a), len(s), pad(a), pad(s), pad(src), pad(h))


def window():
    w = (0.5 + 0.5 * np.cos(np.pi * np.arange(WIN_N + 1, dtype=np.float64) / WIN_N)).astype(np.float32)
    w[WIN_N] = 0.0
    return w


def ola(x, n, p, w_floor=0.5, dtype=np.float32):
    """(y, D): grain by grain in ascending j, so every sample sums its covering grains in ascending j."""
    x = np.asarray(x)
    L, n = len(x), int(n)
    W = window().astype(dtype)
    N, D = np.zeros(L, dtype), np.zeros(L, dtype)
    xs = x[:n].astype(dtype)                                        # nothing at or beyond n is looked at
    for j in range(int(p.J)):
        s, src, h = int(p.s[j]), int(p.src[j]), int(p.h[j])
        lo, hi = max(s - h + 1, 0), min(s + h, n)
        if hi <= lo:
            continue
        d = np.arange(lo, hi) - s
        w = W[(np.abs(d) * WIN_N + h // 2) // h]
        m = src + d
        ok = (m >= 0) & (m < n)
        xv = np.where(ok, xs[np.clip(m, 0, n - 1)], dtype(0))
        N[lo:hi] = N[lo:hi] + (xv * w).astype(dtype)
        D[lo:hi] = D[lo:hi] + w
    y = np.zeros(L, dtype)
    y[:n] = N[:n] / np.maximum(D[:n], dtype(w_floor))
    return y, D


def coverage(L, n, p):
    """G [L] int: the number of grains that cover each sample (0 from n on)."""
    G = np.zeros(L, np.int64)
    for j in range(int(p.J)):
        s, h = int(p.s[j]), int(p.h[j])
        G[max(s - h + 1, 0):min(s + h, int(n))] += 1
    return G


def shift(x, n, period_q, ratio_q, hop, w_floor=0.5, dtype=np.float32):
    p = plan(period_q, ratio_q, n, hop, max_marks(len(x)))
    y, D = ola(x, n, p, w_floor, dtype)
    return y, D, p


def tables(f0, sr, ratio=None, target_f0=None, unvoiced_period=80):
    """(period_q, ratio_q) int32 in the shape of f0, float64 rounded once (ties to even), as conversion.pitch_tables."""
    f0 = np.asarray(f0, dtype=np.float64)
    v = f0 > 0
    per = np.where(v, np.rint(float(sr) * Q / np.where(v, f0, 1.0)), float(int(unvoiced_period) << 16))
    if target_f0 is not None:
        t = np.asarray(target_f0, dtype=np.float64)
        both = v & (t > 0)
        r = np.where(both, np.rint(Q * np.where(both, t, 1.0) / np.where(both, f0, 1.0)), float(Q))
    else:
        r = np.rint(Q * np.broadcast_to(np.asarray(ratio, dtype=np.float64), f0.shape))
    i32 = lambda a: np.clip(a, 0, 2 ** 31 - 1).astype(np.int32)
    return i32(per), i32(r)


def vowel(f0, sr=16000, formants=((700.0, 130.0), (1220.0, 70.0)), amp=0.25):
    """Harmonics of a fundamental given per sample, each weighted by two resonances (centre, bandwidth in Hz) evaluated at
    its own momentary frequency, below sr / 2; float64, scaled to a peak of ``amp``."""
    f0 = np.asarray(f0, np.float64)
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(len(f0))
    for k in range(1, int(0.45 * sr / f0.min()) + 1):
        fk = k * f0
        g = sum(1.0 / np.sqrt(1.0 + ((fk - fc) / bw) ** 2) for fc, bw in formants) + 0.05
        x += np.where(fk < 0.45 * sr, g, 0.0) * np.sin(k * ph + 0.37 * k)
    return amp * x / np.abs(x).max()
