"""The definitions of the content scores in plain numpy (include/vc_hip.h, "Content"), float64 and integers: the
Jensen-Shannon divergence and the arg-max agreement of two posteriorgrams along a set of cells, the phoneme sequence of
a posteriorgram, and the edit distance with the counts its chosen predecessors carry.  Written from the definitions, one
loop per sentence of them; the device is held to this file, not the other way round."""
import numpy as np


def js_bits(p, q):
    """0.5 * sum_c (p log2(p / m) + q log2(q / m)), m = (p + q) / 2, in float64; a term whose p (or q) is <= 0 is 0."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    m = (p + q) / 2.0
    total = 0.0
    for c in range(len(p)):
        if p[c] > 0.0:
            total += p[c] * np.log2(p[c] / m[c])
        if q[c] > 0.0:
            total += q[c] * np.log2(q[c] / m[c])
    return 0.5 * total


def cells_of(len_a, len_b, path=None):
    """The cells the figures run over: the rows of ``path`` (any -1 rows included; they are skipped below) or (i, i)."""
    if path is None:
        return [(i, i) for i in range(min(len_a, len_b))]
    return [(int(i), int(j)) for i, j in np.asarray(path).reshape(-1, 2)]


def ppg_metrics(a, b, len_a, len_b, path=None, class_map=None):
    """dict(n_cells, n_agree, frame_agreement, js_mean) of one pair: a [Fa, C], b [Fb, C]; lengths clamped to [1, F]."""
    len_a, len_b = min(max(int(len_a), 1), len(a)), min(max(int(len_b), 1), len(b))
    n_cells = n_agree = 0
    js = []
    for i, j in cells_of(len_a, len_b, path):
        if not (0 <= i < len_a and 0 <= j < len_b):
            continue
        ka, kb = int(np.argmax(a[i])), int(np.argmax(b[j]))          # numpy's arg-max: the first (lowest) index
        if class_map is not None:
            ka, kb = int(class_map[ka]), int(class_map[kb])
        n_cells += 1
        n_agree += int(ka == kb)
        js.append(js_bits(a[i], b[j]))
    if n_cells == 0:
        return dict(n_cells=0, n_agree=0, frame_agreement=float('nan'), js_mean=float('nan'))
    return dict(n_cells=n_cells, n_agree=n_agree, frame_agreement=n_agree / n_cells, js_mean=float(np.sum(js) / n_cells))


def frame_labels(ppg, n_frames, class_map=None):
    """Step 1: the arg-max of every frame, the lowest index on equality, through the map."""
    F = min(max(int(n_frames), 0), len(ppg))
    lab = [int(np.argmax(ppg[f])) for f in range(F)]
    if class_map is not None:
        lab = [int(class_map[k]) for k in lab]
    return lab


def segments_of_labels(lab, min_run=3):
    """Steps 2 to 5 on a list of frame labels; returns (labels, start, end) lists, end exclusive."""
    runs = []                                                       # 2. maximal stretches of equal labels
    for f, k in enumerate(lab):
        if runs and runs[-1][0] == k:
            runs[-1][2] = f + 1
        else:
            runs.append([k, f, f + 1])
    runs = [r for r in runs if r[2] - r[1] >= min_run]              # 3. short runs leave
    merged = []                                                     # 4. equal neighbours merge, once
    for k, s, e in runs:
        if merged and merged[-1][0] == k:
            merged[-1][2] = e
        else:
            merged.append([k, s, e])
    kept = [m for m in merged if m[0] != -1]                        # 5. dropped classes leave; nothing merges after that
    return [m[0] for m in kept], [m[1] for m in kept], [m[2] for m in kept]


def phn_segments(ppg, n_frames, class_map=None, min_run=3):
    return segments_of_labels(frame_labels(ppg, n_frames, class_map), min_run)


def padded_segments(ppg, n_frames, max_frames, class_map=None, min_run=3):
    """The device's row layout: three int32 [max_frames] arrays, -1 from the count on, and the count."""
    lab, st, en = phn_segments(ppg, n_frames, class_map, min_run)
    out = np.full((3, max_frames), -1, dtype=np.int32)
    out[0, :len(lab)], out[1, :len(lab)], out[2, :len(lab)] = lab, st, en
    return out[0], out[1], out[2], len(lab)


def edit_distance(a, b):
    """dict(dist, n_match, n_sub, n_del, n_ins, per) of two sequences.  Every cell holds (E, n_match, n_sub, n_del, n_ins)
    taken from its chosen predecessor; on equal costs the order is diagonal, up, left."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    prev = [(j, 0, 0, 0, j) for j in range(len(b) + 1)]             # E(0, j) = j: insertions
    for i in range(1, len(a) + 1):
        row = [(i, 0, 0, i, 0)]                                     # E(i, 0) = i: deletions
        for j in range(1, len(b) + 1):
            dg, up, lf = prev[j - 1], prev[j], row[j - 1]
            sub = a[i - 1] != b[j - 1]
            best = (dg[0] + sub, dg[1] + (not sub), dg[2] + sub, dg[3], dg[4])
            if up[0] + 1 < best[0]:
                best = (up[0] + 1, up[1], up[2], up[3] + 1, up[4])
            if lf[0] + 1 < best[0]:
                best = (lf[0] + 1, lf[1], lf[2], lf[3], lf[4] + 1)
            row.append(best)
        prev = row
    E, m, s, d, n = (int(v) for v in prev[len(b)])
    assert E == s + d + n and m + s + d == len(a)
    return dict(dist=E, n_match=m, n_sub=s, n_del=d, n_ins=n, per=E / len(a) if a else float('nan'))
