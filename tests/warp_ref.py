"""Restatement of the duration map and the time warp (include/vc_hip.h, "Duration") in numpy.

The map is integer arithmetic throughout (python integers, so no width is assumed), and the warp is three separately
rounded float32 operations per element, so the device is compared against both bit for bit.

  duration_map(n, start, end, n_seg, ...)   -> Map(pos [Fw_max] int32, n_out, out_start, out_end [K] int32, flags)
  duration_map_batch(...)                   the same for a ragged batch
  time_warp(x [F, C] float32, pos, n_out, n, mode)   -> [Fw_max, C] float32
  center_map_f64(pieces)                    the float64 centre-aligned map S + (j + 1/2) Li / Lo - 1/2 the formula stands for
  pieces(n, start, end, n_seg, ...)         the piece table (S, Li, O, Lo, segment index or -1) of a VALID table, or None
"""
from collections import namedtuple

import numpy as np

Q = 65536
RATIO_MAX_Q = 8 * Q
FLAG_INVALID, FLAG_SHORT, FLAG_TRUNCATED = 1, 2, 4
Map = namedtuple('duration_map', 'pos n_out out_start out_end flags')


def ratio_to_q(ratio):
    """float ratios -> Q16 int32 as conversion.duration_map_batch rounds them: float32, times 65536 (exact), to the nearest
    integer with ties to even, clamped to [0, 8 * 65536]."""
    r = np.rint(np.asarray(ratio, dtype=np.float32) * np.float32(Q))
    return np.clip(r, 0, RATIO_MAX_Q).astype(np.int32)


def scaled(Li, q):
    q = min(max(int(q), 0), RATIO_MAX_Q)
    return (int(Li) * q + 32768) >> 16


def pieces(n, start, end, n_seg, labels=None, out_len=None, ratio_q=None, gap_q=Q):
    """The pieces of a valid table in input order: a list of (S, Li, O, Lo, k) with k the table entry of a segment and -1
    for a gap (gaps of no frames included: they have Li = Lo = 0); None for an invalid table."""
    n, n_seg = int(n), int(n_seg)
    prev, O, out = 0, 0, []

    def add(S, Li, Lo, k):
        nonlocal O
        out.append((S, Li, O, Lo, k))
        O += Lo

    for k in range(n_seg):
        s, e = int(start[k]), int(end[k])
        if s < 0 or e == s:
            continue                                                # absent
        if e < s or s < prev or e > n:
            return None
        if out_len is not None:
            Lo = int(out_len[k])
            if Lo < 0:
                return None
        elif ratio_q is not None and labels is not None:
            c = int(labels[k])
            if c < 0 or c >= len(ratio_q):
                return None
            Lo = scaled(e - s, ratio_q[c])
        elif ratio_q is not None:
            Lo = scaled(e - s, ratio_q[0])                          # without labels: one rate for every segment
        else:
            Lo = e - s
        add(prev, s - prev, scaled(s - prev, gap_q), -1)
        add(s, e - s, Lo, k)
        prev = e
    add(prev, n - prev, scaled(n - prev, gap_q), -1)
    return out


def piece_pos(S, Li, Lo, j, n):
    p = S * Q + ((2 * j + 1) * Li * Q) // (2 * Lo) - 32768
    return min(max(p, 0), (n - 1) * Q)


def duration_map(n, start, end, n_seg, labels=None, out_len=None, ratio_q=None, gap_q=Q, min_frames=1, Fw_max=None):
    """One utterance.  start, end (, labels, out_len): [K] integers; n_seg is clamped to [0, K].  pos is -1 from n_out on;
    out_start / out_end are -1 for absent entries, from n_seg on, for an invalid table and for n == 0."""
    n = int(n)
    K = len(start)
    n_seg = min(max(int(n_seg), 0), K)
    Fw_max = n if Fw_max is None else int(Fw_max)
    pos = np.full((Fw_max,), -1, np.int32)
    o_s, o_e = np.full((K,), -1, np.int32), np.full((K,), -1, np.int32)
    if n <= 0:
        return Map(pos, 0, o_s, o_e, 0)
    P = pieces(n, start, end, n_seg, labels, out_len, ratio_q, gap_q)
    flags = 0
    if P is None:
        flags |= FLAG_INVALID
    else:
        total = sum(p[3] for p in P)
        if total < int(min_frames):
            flags |= FLAG_SHORT
    if flags:                                                       # the identity map
        if P is None:
            P = []
        else:                                                       # a valid table stays what it was
            P = [(S, Li, S, Li, k) for S, Li, O, Lo, k in P]
        total = n
        if total > Fw_max:
            flags |= FLAG_TRUNCATED
        n_out = min(total, Fw_max)
        pos[:n_out] = np.arange(n_out, dtype=np.int64) * Q
    else:
        if total > Fw_max:
            flags |= FLAG_TRUNCATED
        n_out = min(total, Fw_max)
        for S, Li, O, Lo, k in P:
            for u in range(O, min(O + Lo, n_out)):
                pos[u] = piece_pos(S, Li, Lo, u - O, n)
    for S, Li, O, Lo, k in P:
        if k >= 0:
            o_s[k], o_e[k] = min(O, n_out), min(O + Lo, n_out)
    return Map(pos, n_out, o_s, o_e, flags)


def duration_map_batch(lens, start, end, n_seg, labels=None, out_len=None, ratio_q=None, gap_q=Q, min_frames=1, Fw_max=None):
    B = len(lens)
    Fw_max = int(max(lens)) if Fw_max is None else int(Fw_max)
    rows = [duration_map(lens[b], start[b], end[b], n_seg[b], None if labels is None else labels[b],
                         None if out_len is None else out_len[b], ratio_q, gap_q, min_frames, Fw_max) for b in range(B)]
    return Map(np.stack([r.pos for r in rows]), np.array([r.n_out for r in rows], np.int32), np.stack([r.out_start for r in rows]),
               np.stack([r.out_end for r in rows]), np.array([r.flags for r in rows], np.int32))


def center_map_f64(P):
    """The centre-aligned map in float64, unclamped: frame j of a piece reads S + (j + 1/2) Li / Lo - 1/2."""
    out = []
    for S, Li, O, Lo, k in P:
        j = np.arange(Lo, dtype=np.float64)
        out.append(S + (j + 0.5) * (Li / Lo if Lo else 0.0) - 0.5)
    return np.concatenate(out) if out else np.zeros((0,))


def time_warp(x, pos, n_out, n, mode='linear'):
    """x [F, C] float32, pos [Fw] int32 (Q16 frames), n input frames -> [Fw, C] float32; rows from n_out on are zero.  pos is
    clamped to [0, (n - 1) * 65536] before use, as the device does with every value it reads."""
    x = np.asarray(x, dtype=np.float32)
    Fw = len(pos)
    out = np.zeros((Fw, x.shape[1]), np.float32)
    n, n_out = min(max(int(n), 0), x.shape[0]), min(max(int(n_out), 0), Fw)
    if n == 0 or n_out == 0:
        return out
    p = np.clip(np.asarray(pos[:n_out], dtype=np.int64), 0, (n - 1) * Q)
    if mode == 'nearest':
        out[:n_out] = x[np.minimum((p + 32768) >> 16, n - 1)]
        return out
    i0 = p >> 16
    i1 = np.minimum(i0 + 1, n - 1)
    w = ((p & 65535).astype(np.float32) * np.float32(2.0 ** -16))[:, None]
    a, b = x[i0], x[i1]
    d = (b - a).astype(np.float32)
    m = (w * d).astype(np.float32)
    v = (a + m).astype(np.float32)
    out[:n_out] = np.where(w == 0, a, v)
    return out
