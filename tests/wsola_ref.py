"""Restatement of waveform time scaling (include/vc_hip.h, "Time scale") in numpy.

Waveform-similarity overlap-add: grains of 2 S samples are copied from the input, one every S output samples; each is
chosen within +-tol samples of where the time map points so that it continues its predecessor (least sum of absolute
differences on the signal quantised to 16 bits).  Every decision is integer arithmetic (python integers / int64, so no
width is assumed); the overlap-add is three rounded operations per sample in the working dtype.  The device is compared
against the float32 reading bit for bit.

  quantise(x, qscale)                        q [len(x)] int64 in [-32767, 32767]
  sizes(n_out, n, hop, S)                    -> (out_len, K)
  max_grains(out_frames, hop, S)             the row length of a plan
  targets(pos, n_out, n, hop, g)             tau [K] (python integers)
  plan(x, n, pos, n_out, hop, g, tol, ...)   -> Plan(K, out_len, a, cost [M], tau [K])
  window(S)                                  T [S] float32
  ola(x, n, a, n_grains, out_len, S, L)      -> y [L]
  scale(x, n, pos, n_out, hop, ...)          plan + ola -> (y, plan)
  rate_map(n_frames, rate) / identity_map(n) uniform Q16 maps with the -1 padding of vc_duration_map
"""
from collections import namedtuple

import numpy as np

Q = 65536
A_GUARD = 1 << 24
A_PAD = -2 ** 31
Plan = namedtuple('wsola_plan', 'K out_len a cost tau')


def quantise(x, qscale=32768.0):
    """clamp(rint(float32(x * qscale)), -32767, 32767): one float32 product, rounded half to even; NaN -> 0."""
    with np.errstate(over='ignore', invalid='ignore'):
        p = np.asarray(x, np.float32) * np.float32(qscale)
        r = np.rint(p)
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, -32767, 32767).astype(np.int64)


def sizes(n_out, n, hop, S):
    out_len = int(hop) * (int(n_out) - 1) if n_out >= 2 and n >= 1 else 0
    K = -(-out_len // int(S)) + 1 if out_len > 0 else 0
    return out_len, K


def max_grains(out_frames, hop, S):
    return -(-(int(hop) * (int(out_frames) - 1)) // int(S)) + 1


def targets(pos, n_out, n, hop, g, K):
    out = []
    for k in range(K):
        u = min(k * g, n_out - 1)
        p = max(int(pos[u]), 0)
        out.append(min(max((p * hop + 32768) >> 16, 0), n - 1))
    return out


def _ext(v, lo, count):
    """v~[lo .. lo + count): v extended by zeros on both sides."""
    n = len(v)
    out = np.zeros(count, v.dtype)
    s, e = max(lo, 0), min(lo + count, n)
    if e > s:
        out[s - lo:e - lo] = v[s:e]
    return out


def plan(x, n, pos, n_out, hop, g=2, tol=None, qscale=32768.0, max_len=None, out_frames=None, M=None):
    """The grain positions of one utterance.  n is clamped to [0, max_len] (default len(x)), n_out to [0, out_frames]
    (default len(pos)); nothing of x at or beyond n and nothing of pos at or beyond n_out is looked at."""
    hop, g = int(hop), int(g)
    S = g * hop
    tol = S if tol is None else int(tol)
    n = min(max(int(n), 0), len(x) if max_len is None else int(max_len))
    F = len(pos) if out_frames is None else int(out_frames)
    n_out = min(max(int(n_out), 0), F)
    M = max_grains(F, hop, S) if M is None else int(M)
    out_len, K = sizes(n_out, n, hop, S)
    q = quantise(np.asarray(x)[:n], qscale)
    tau = targets(pos, n_out, n, hop, g, K)
    a, cost = [], []
    d_all = np.arange(-tol, tol + 1)
    for k in range(K):
        if k == 0:
            a.append(tau[0]); cost.append(0)
            continue
        ref = _ext(q, a[-1], 2 * S)                                 # q~[n_k - S .. n_k + S), n_k = a_{k-1} + S
        span = _ext(q, tau[k] - tol - S, 2 * S + 2 * tol)
        c = np.abs(np.lib.stride_tricks.sliding_window_view(span, 2 * S) - ref[None, :]).sum(axis=1)
        key = min(zip(c.tolist(), np.abs(d_all).tolist(), d_all.tolist()))
        a.append(tau[k] + key[2]); cost.append(key[0])
    pad = lambda v, fill: np.array(list(v) + [fill] * (M - len(v)), dtype=np.int64).astype(np.int32)
    return Plan(K, out_len, pad(a, A_PAD), pad(cost, -1), tau)


def window(S):
    return (0.5 - 0.5 * np.cos(np.pi * np.arange(int(S), dtype=np.float64) / int(S))).astype(np.float32)


def ola(x, n, a, n_grains, out_len, S, L, dtype=np.float32, max_len=None):
    """y [L]: y[m] = A + T[r] * (B - A), three rounded operations.  The plan is read as the launch reads it: n_grains is
    clamped to the row, out_len to [0, L]; a grain at or beyond n_grains, or whose a lies outside [-2^24, 2^24], covers
    nothing (its samples count as 0)."""
    S, L = int(S), int(L)
    n = min(max(int(n), 0), len(x) if max_len is None else int(max_len))
    n_grains = min(max(int(n_grains), 0), len(a))
    out_len = min(max(int(out_len), 0), L)
    xs = np.asarray(x)[:n].astype(dtype)
    T = window(S).astype(dtype)
    y = np.zeros(L, dtype)
    if out_len == 0:
        return y
    m = np.arange(out_len)
    k, r = m // S, m % S

    def take(kk, off):
        ok = kk < n_grains
        av = np.asarray(a, np.int64)[np.minimum(kk, max(n_grains - 1, 0))] if n_grains else np.zeros(len(kk), np.int64)
        ok = ok & (av >= -A_GUARD) & (av <= A_GUARD)
        idx = av + off
        ok = ok & (idx >= 0) & (idx < n)
        v = xs[np.clip(idx, 0, max(n - 1, 0))] if n else np.zeros(len(kk), dtype)
        return np.where(ok, v, dtype(0)).astype(dtype)

    A, B = take(k, r), take(k + 1, r - S)
    with np.errstate(over='ignore', invalid='ignore'):
        d = (B - A).astype(dtype)
        y[:out_len] = A + (T[r] * d).astype(dtype)
    return y


def scale(x, n, pos, n_out, hop, g=2, tol=None, qscale=32768.0, dtype=np.float32):
    p = plan(x, n, pos, n_out, hop, g, tol, qscale)
    L = int(hop) * (len(pos) - 1)
    return ola(x, n, p.a, p.K, p.out_len, int(g) * int(hop), L, dtype), p


def identity_map(n_frames, F=None):
    F = n_frames if F is None else F
    pos = np.full(F, -1, np.int32)
    pos[:n_frames] = np.arange(n_frames, dtype=np.int64) << 16
    return pos


def rate_map(n_frames, rate, F=None):
    """One piece [0, n_frames) at ``rate``: Lo = round(n_frames * rate) output frames; output frame u reads input frame
    u * n_frames / Lo (Q16, rounded down) -- a uniform monotone map, -1 from Lo on.  Returns (pos [F], Lo)."""
    Lo = int(np.rint(n_frames * float(rate)))
    F = Lo if F is None else F
    pos = np.full(F, -1, np.int32)
    u = np.arange(Lo, dtype=np.int64)
    pos[:Lo] = np.minimum((u * n_frames * Q) // max(Lo, 1), (n_frames - 1) * Q)
    return pos, Lo
