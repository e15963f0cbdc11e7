"""Forced alignment (include/vc_hip.h, "Alignment") restated in numpy: the yardstick of tests/test_align_*.py.

Per utterance: score [F, C] float32 (finite or -inf; callers pass log-posteriors), seq [S] class indices, opt [S] (1 =
the state may be skipped) or None.

    e(t, s) = score[t, seq[s]], -inf when seq[s] lies outside [0, C)
    D(0, s) = e(0, s) for s = 0, and for s = 1 iff opt[0]; -inf otherwise
    D(t, s) = e(t, s) + best;  best = D(t-1, s)                              (stay, code 0)
                               replaced by D(t-1, s-1) iff strictly greater  (advance, code 1)
                               then by D(t-1, s-2) iff opt[s-1] and strictly greater (skip, code 2)
    final   = S-1, or S-2 iff S >= 2, opt[S-1] and D(F-1, S-2) > D(F-1, S-1);  total = D(F-1, final)
    infeasible: F == 0, S == 0 or total == -inf

The path is read back from the codes, mechanically, from (F-1, final) to frame 0, whatever the values are (with a NaN in
the scores the walk may end in a state that D(0, .) does not admit; it is still THE path of this definition).

align_f32      float32, one IEEE add and strict compare-selects per cell: what the device must equal bit for bit
align_f64      the same recurrence in float64 (the optimum against which the float32 path's cost is bounded)
brute_force    every admissible monotone path of a tiny problem, scored by adding the emissions in frame order
"""
from collections import namedtuple
import itertools

import numpy as np

Alignment = namedtuple('Alignment', 'frame_state start end seg_score total n_visited')
NEG = -np.inf


def emissions(score, seq, dtype=np.float32):
    """e [F, S]: score[:, seq[s]], -inf for a class outside [0, C)."""
    score = np.asarray(score)
    F, C = score.shape
    seq = np.asarray(seq, dtype=np.int64)
    ok = (seq >= 0) & (seq < C)
    e = np.full((F, len(seq)), NEG, dtype=dtype)
    if ok.any():
        e[:, ok] = score[:, seq[ok]].astype(dtype)
    return e


def _forward(e, opt):
    """D of the last frame and the codes [F, S] (row 0 all zero).  Sequential over frames, elementwise over states."""
    F, S = e.shape
    dt = e.dtype.type
    neg = dt(NEG)
    d = np.full((S,), neg, dtype=e.dtype)
    d[0] = e[0, 0]
    if S > 1 and opt[0]:
        d[1] = e[0, 1]
    codes = np.zeros((F, S), dtype=np.uint8)
    skip_ok = np.zeros((S,), dtype=bool)          # skip INTO s: opt[s-1], s >= 2
    skip_ok[2:] = opt[1:S - 1].astype(bool)
    with np.errstate(invalid='ignore'):
        for t in range(1, F):
            p1 = np.concatenate([[neg], d[:-1]]).astype(e.dtype)
            p2 = np.concatenate([[neg, neg], d[:-2]]).astype(e.dtype)[:S]
            best, code = d.copy(), np.zeros((S,), dtype=np.uint8)
            a = p1 > best
            best[a], code[a] = p1[a], 1
            k = skip_ok & (p2 > best)
            best[k], code[k] = p2[k], 2
            d = (e[t] + best).astype(e.dtype)
            codes[t] = code
    return d, codes


def _walk(e, codes, final, S_max, F_max):
    F, S = e.shape
    frame_state = np.full((F_max,), -1, dtype=np.int32)
    start = np.full((S_max,), -1, dtype=np.int32)
    end = np.full((S_max,), -1, dtype=np.int32)
    seg = np.full((S_max,), np.nan, dtype=np.float32)
    s = final
    end[s] = F
    for t in range(F - 1, -1, -1):
        frame_state[t] = s
        start[s] = t
        c = int(codes[t, s]) if t > 0 else 0
        if c:
            s -= c
            end[s] = t
    for s in np.nonzero(start >= 0)[0]:
        acc = np.float64(0.0)
        for t in range(start[s], end[s]):
            acc = acc + np.float64(e[t, s])
        seg[s] = np.float32(acc / np.float64(end[s] - start[s]))
    return frame_state, start, end, seg, int((start >= 0).sum())


def _align(score, seq, opt, n_frames, n_seq, dtype):
    score = np.asarray(score)
    F_max = score.shape[0]
    seq = np.asarray(seq)
    S_max = len(seq)
    F = int(min(max(n_frames if n_frames is not None else F_max, 0), F_max))
    S = int(min(max(n_seq if n_seq is not None else S_max, 0), S_max))
    opt = np.zeros((S_max,), dtype=np.uint8) if opt is None else (np.asarray(opt) != 0).astype(np.uint8)
    none = Alignment(np.full((F_max,), -1, np.int32), np.full((S_max,), -1, np.int32), np.full((S_max,), -1, np.int32),
                     np.full((S_max,), np.nan, np.float32), dtype(NEG), 0)
    if F == 0 or S == 0:
        return none
    e = emissions(score[:F], seq[:S], dtype)
    d, codes = _forward(e, opt[:S])
    final = S - 1
    if S >= 2 and opt[S - 1] and d[S - 2] > d[S - 1]:
        final = S - 2
    total = d[final]
    if total == dtype(NEG):
        return none
    fs, st, en, seg, nv = _walk(e, codes, final, S_max, F_max)
    return Alignment(fs, st, en, seg, dtype(total), nv)


def align_f32(score, seq, opt=None, n_frames=None, n_seq=None):
    """One utterance, float32.  score [F_max, C], seq [S_max]; outputs padded to F_max / S_max with the defined fill."""
    return _align(np.asarray(score, dtype=np.float32), seq, opt, n_frames, n_seq, np.float32)


def align_f64(score, seq, opt=None, n_frames=None, n_seq=None):
    return _align(np.asarray(score, dtype=np.float64), seq, opt, n_frames, n_seq, np.float64)


def align_batch_f32(score, seq, opt, n_frames, n_seq):
    """score [B, F_max, C], seq [B, S_max], opt [B, S_max] or None, lengths [B] -> Alignment of stacked arrays."""
    rows = [align_f32(score[b], seq[b], None if opt is None else opt[b], int(n_frames[b]), int(n_seq[b])) for b in range(len(score))]
    return Alignment(*(np.stack([np.asarray(getattr(r, f)) for r in rows]) for f in Alignment._fields))


def path_cost_f64(score, seq, frame_state):
    """The cost of a path (frame_state [F], every entry >= 0) in float64, the emissions added in frame order."""
    e = emissions(np.asarray(score, dtype=np.float64), seq, np.float64)
    acc = np.float64(0.0)
    for t, s in enumerate(frame_state):
        acc = acc + e[t, s]
    return acc


def admissible_paths(F, S, opt):
    """Every state sequence of F frames over S states that starts in an admitted state, moves by 0, 1 or (over an optional
    state) 2, and ends in an admitted state.  In the order of preference of the tie rule: see brute_force."""
    opt = [bool(o) for o in opt]
    first = [0] + ([1] if S > 1 and opt[0] else [])
    last = [S - 1] + ([S - 2] if S > 1 and opt[S - 1] else [])
    out = []
    for steps in itertools.product((0, 1, 2), repeat=F - 1):
        for s0 in first:
            s, path, ok = s0, [s0], True
            for c in steps:
                s += c
                if s >= S or (c == 2 and not opt[s - 1]):
                    ok = False
                    break
                path.append(s)
            if ok and s in last:
                out.append(path)
    return out


def brute_force(score, seq, opt=None):
    """(best total, the set of optimal paths) over every admissible path, float32 partial sums in frame order.  On
    integer-valued scores every sum is exact, so the optimum is THE optimum and equal totals are true ties."""
    score = np.asarray(score, dtype=np.float32)
    F = score.shape[0]
    S = len(seq)
    opt = [0] * S if opt is None else list(opt)
    e = emissions(score, seq, np.float32)
    best, arg = np.float32(NEG), []
    for p in admissible_paths(F, S, opt):
        acc = e[0, p[0]]
        for t in range(1, F):
            acc = np.float32(acc + e[t, p[t]])
        if acc > best:
            best, arg = acc, [p]
        elif acc == best and acc != np.float32(NEG):
            arg.append(p)
    return best, arg


def tie_choice(paths, S):
    """Which of several optimal paths the recurrence's strict compares return.  Read backwards from the last frame: the
    final state S-1 unless only S-2 is optimal...  the rule is local, so it is restated here on the SET of optimal paths:
    at the end prefer S-1 (S-2 only wins when strictly greater); going back, at each frame prefer stay, then advance, then
    skip, among the predecessors that still lie on an optimal path THROUGH the current cell.  Valid on exact (integer)
    scores, where 'lies on an optimal path' and 'has the greatest D' say the same thing."""
    F = len(paths[0])
    alive = [tuple(p) for p in paths]
    s = S - 1 if any(p[-1] == S - 1 for p in alive) else S - 2
    alive = [p for p in alive if p[-1] == s]
    out = [s]
    for t in range(F - 1, 0, -1):
        for c in (0, 1, 2):
            nxt = [p for p in alive if p[t - 1] == s - c]
            if nxt:
                alive, s = nxt, s - c
                break
        out.append(s)
    return out[::-1]


def synthetic_posteriors(seg_labels, seg_lens, n_classes, seed=0, peak=0.9, smooth=2, noise=0.02):
    """Speech-like posteriors [F, C] from a known segmentation: one-hot at ``peak`` (the rest spread evenly), smoothed along
    time by a box of 2 * smooth + 1 frames, plus uniform noise of amplitude ``noise``, renormalised."""
    rng = np.random.RandomState(seed)
    lab = np.repeat(np.asarray(seg_labels), np.asarray(seg_lens))
    F = len(lab)
    p = np.full((F, n_classes), (1.0 - peak) / max(n_classes - 1, 1))
    p[np.arange(F), lab] = peak
    if smooth:
        pad = np.concatenate([np.repeat(p[:1], smooth, 0), p, np.repeat(p[-1:], smooth, 0)])
        p = sum(pad[k:k + F] for k in range(2 * smooth + 1)) / (2 * smooth + 1)
    p = p + noise * rng.rand(F, n_classes)
    p /= p.sum(1, keepdims=True)
    return p.astype(np.float32)
