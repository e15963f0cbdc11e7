"""Phone-loop Viterbi decoding (include/vc_hip.h, "Decoding") restated in numpy: the yardstick of tests/test_decode_*.py.

Per utterance: score [F, C] (finite or -inf), trans [C, C] (trans[i, j] is added when a segment of class i ends and one of
class j begins; i == j is an ordinary entry), init / final [C] or None, min_dur M in [1, 8], class_map [C] or None.

States (c, d), d = 0 .. M-1: class c in its (d+1)-th frame, or later when d = M-1.  e(t, c) = score[t, c].

    D(0, (c, 0)) = init[c] + e(0, c)   (without init: e(0, c));   D(0, (c, d > 0)) = -inf
    X(t, c)      = max over i ascending of fl(D(t-1, (i, M-1)) + trans[i, c]); a later i replaces the holder only when
                   strictly greater; bp(t, c) is the holder's i
    M = 1:  D(t, (c, 0)) = e(t, c) + best, best = D(t-1, (c, 0)) (stay), replaced by X(t, c) (enter) iff strictly greater
    M > 1:  D(t, (c, 0)) = e(t, c) + X(t, c);  D(t, (c, d)) = e(t, c) + D(t-1, (c, d-1)) for 0 < d < M-1;
            D(t, (c, M-1)) = e(t, c) + best, best = D(t-1, (c, M-1)) (stay), replaced by D(t-1, (c, M-2)) (advance) iff
            strictly greater
    total = max over c ascending of D(F-1, (c, M-1)) + final[c] (without final: the bare value), the lowest c on a tie
    infeasible: F == 0, F < M or total == -inf

The moves of a frame fit one byte per class: bits 0-6 bp(t, c), bit 7 the second choice into the last state (advance;
enter when M = 1).  The path is read back from them, mechanically, from (F-1, (c*, M-1)).

decode_f32     float32, one IEEE add per term and strict compares: what the device must equal bit for bit
decode_f64     the same recurrence in float64 (the optimum against which the float32 path's cost is bounded)
brute_force    every segmentation and labelling of a tiny problem
"""
from collections import namedtuple
import itertools

import numpy as np

Decoded = namedtuple('Decoded', 'frame_class seg_label seg_start seg_end n_seg seg_score total raw')
NEG = -np.inf
MAX_DUR = 8


def _forward(e, trans, init, final, M):
    """(total, last class, moves [F, C] uint8).  Sequential over frames, elementwise over classes."""
    F, C = e.shape
    dt = e.dtype
    cols = np.arange(C)
    D = np.full((M, C), NEG, dtype=dt)
    D[0] = e[0] if init is None else (init + e[0]).astype(dt)
    moves = np.zeros((F, C), dtype=np.uint8)
    with np.errstate(invalid='ignore'):
        for t in range(1, F):
            terms = (D[M - 1][:, None] + trans).astype(dt)          # [i, c], each rounded before the compare
            bp = terms.argmax(0)                                    # the first of the greatest: the lowest i on a tie
            X = terms[bp, cols]
            stay = D[M - 1]
            cand = X if M == 1 else D[M - 2]
            bit = cand > stay
            last = (e[t] + np.where(bit, cand, stay)).astype(dt)
            new = np.empty_like(D)
            if M > 1:
                new[0] = (e[t] + X).astype(dt)
                for d in range(1, M - 1):
                    new[d] = (e[t] + D[d - 1]).astype(dt)
            new[M - 1] = last
            D = new
            moves[t] = bp.astype(np.uint8) | (bit.astype(np.uint8) << 7)
    end = D[M - 1] if final is None else (D[M - 1] + final).astype(dt)
    c = int(end.argmax())
    return end[c], c, moves


def _walk(moves, c, F, M):
    """The decoded segments [(class, start, end)] in frame order."""
    segs, d, stop = [], M - 1, F
    for t in range(F - 1, 0, -1):
        m = int(moves[t, c])
        if M > 1 and d == M - 1:
            d = M - 2 if m & 128 else M - 1
        elif d > 0:
            d -= 1
        elif M > 1 or m & 128:                                      # the segment was entered at t
            segs.append((c, t, stop))
            stop, c, d = t, m & 127, M - 1
    segs.append((c, 0, stop))
    return segs[::-1]


def segments(raw, class_map):
    """Decoded segments -> labels through class_map -> equal neighbours merged -> segments labelled -1 dropped."""
    out = []
    for c, s, e in raw:
        lab = int(c if class_map is None else class_map[c])
        if out and out[-1][0] == lab:
            out[-1][2] = e
        else:
            out.append([lab, s, e])
    return [tuple(s) for s in out if s[0] != -1]


def _decode(score, trans, init, final, min_dur, class_map, n_frames, dtype):
    score = np.asarray(score, dtype=dtype)
    F_max, C = score.shape
    M = int(min_dur)
    assert 1 <= M <= MAX_DUR and 1 <= C <= 128
    F = int(min(max(F_max if n_frames is None else n_frames, 0), F_max))
    trans = np.asarray(trans, dtype=dtype)
    init = None if init is None else np.asarray(init, dtype=dtype)
    final = None if final is None else np.asarray(final, dtype=dtype)
    none = Decoded(np.full((F_max,), -1, np.int32), np.full((F_max,), -1, np.int32), np.full((F_max,), -1, np.int32),
                   np.full((F_max,), -1, np.int32), 0, np.full((F_max,), np.nan, np.float32), dtype(NEG), [])
    if F == 0 or F < M:
        return none
    total, c, moves = _forward(score[:F], trans, init, final, M)
    if total == dtype(NEG):
        return none
    raw = _walk(moves, c, F, M)
    frame_class = np.full((F_max,), -1, np.int32)
    for k, s, e in raw:
        frame_class[s:e] = k
    segs = segments(raw, class_map)
    lab, st, en = (np.full((F_max,), -1, np.int32) for _ in range(3))
    sc = np.full((F_max,), np.nan, np.float32)
    for n, (k, s, e) in enumerate(segs):
        lab[n], st[n], en[n] = k, s, e
        acc = np.float64(0.0)
        for t in range(s, e):
            acc = acc + np.float64(score[t, frame_class[t]])
        sc[n] = np.float32(acc / np.float64(e - s))
    return Decoded(frame_class, lab, st, en, len(segs), sc, dtype(total), raw)


def decode_f32(score, trans, init=None, final=None, min_dur=3, class_map=None, n_frames=None):
    """One utterance, float32.  score [F_max, C]; outputs padded to F_max with the defined fill."""
    return _decode(score, trans, init, final, min_dur, class_map, n_frames, np.float32)


def decode_f64(score, trans, init=None, final=None, min_dur=3, class_map=None, n_frames=None):
    return _decode(score, trans, init, final, min_dur, class_map, n_frames, np.float64)


def decode_batch_f32(score, n_frames, trans, init=None, final=None, min_dur=3, class_map=None):
    """score [B, F_max, C], n_frames [B] -> Decoded of stacked arrays (raw: a list per utterance)."""
    rows = [decode_f32(score[b], trans, init, final, min_dur, class_map, int(n_frames[b])) for b in range(len(score))]
    return Decoded(*(np.stack([np.asarray(getattr(r, f)) for r in rows]) for f in Decoded._fields[:-1]), [r.raw for r in rows])


def path_cost_f64(score, trans, init, final, raw):
    """The cost of a segmentation [(class, start, end)] in float64, added in frame order as the recurrence adds."""
    score, trans = np.asarray(score, dtype=np.float64), np.asarray(trans, dtype=np.float64)
    acc = np.float64(0.0)
    for n, (c, s, e) in enumerate(raw):
        if n == 0:
            acc = score[0, c] if init is None else np.float64(init[c]) + score[0, c]
        else:
            acc = score[s, c] + (acc + trans[raw[n - 1][0], c])
        for t in range(s + 1, e):
            acc = score[t, c] + acc
    return acc if final is None else acc + np.float64(final[raw[-1][0]])


def raw_from_frames(frame_class):
    """The segmentation of a path without repeated classes (a trans with a -inf diagonal): the runs of frame_class."""
    fc = np.asarray(frame_class)
    cuts = [0] + [t for t in range(1, len(fc)) if fc[t] != fc[t - 1]] + [len(fc)]
    return [(int(fc[a]), a, b) for a, b in zip(cuts[:-1], cuts[1:])]


def brute_force(score, trans, init=None, final=None, min_dur=1):
    """The best total over every segmentation of the F frames into segments of at least min_dur frames and every
    labelling of the segments.  On integer-valued scores every sum is exact, so it is THE optimum."""
    score = np.asarray(score, dtype=np.float32)
    F, C = score.shape
    best = np.float32(NEG)

    def splits(left):
        if left == 0:
            yield []
        for n in range(min_dur, left + 1):
            for rest in splits(left - n):
                yield [n] + rest

    for lens in splits(F):
        cuts = np.concatenate([[0], np.cumsum(lens)])
        for labs in itertools.product(range(C), repeat=len(lens)):
            raw = [(c, int(cuts[k]), int(cuts[k + 1])) for k, c in enumerate(labs)]
            v = np.float32(path_cost_f64(score, trans, init, final, raw))
            if v > best:
                best = v
    return best


def edit_distance(a, b):
    """Levenshtein distance of two sequences, unit costs."""
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j - 1] + (x != y), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[-1]


def argmax_segments(p, min_run=3, class_map=None):
    """vc_phn_segments restated: arg-max labels, runs shorter than min_run removed, equal neighbours merged, -1 dropped."""
    lab = np.asarray(p).argmax(1)
    if class_map is not None:
        lab = np.asarray(class_map)[lab]
    runs = [(int(c), a, b) for c, a, b in raw_from_frames(lab) if b - a >= min_run]
    return segments(runs, None)


def phn_transitions(seqs, n_seq, n_classes, add=1.0, scale=1.0, allow_repeat=False):
    """evaluation.phn_transitions restated with explicit loops (float64 counts)."""
    C = int(n_classes)
    cnt = np.zeros((C, C), np.float64)
    for s, n in zip(seqs, n_seq):
        for k in range(int(n) - 1):
            cnt[int(s[k]), int(s[k + 1])] += 1.0
    with np.errstate(divide='ignore'):
        out = scale * np.log((cnt + add) / (cnt.sum(1, keepdims=True) + add * C))
    if not allow_repeat:
        out[np.arange(C), np.arange(C)] = NEG
    return out.astype(np.float32)
