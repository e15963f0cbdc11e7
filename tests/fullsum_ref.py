"""Full-sum alignment (include/vc_hip.h, "Alignment", second half) restated in float64 numpy: the yardstick of
tests/test_fullsum_*.py.

Per utterance: score [F, C] (finite or -inf; callers pass log-posteriors), seq [S] class indices, opt [S] (1 = the state
may be skipped) or None.  The lattice is forced alignment's (tests/align_ref.py):

    e(t, s)     = score[t, seq[s]], -inf when seq[s] lies outside [0, C)
    la(0, s)    = e(0, s) for s = 0, and for s = 1 iff opt[0]; -inf otherwise
    la(t, s)    = e(t, s) + lse(la(t-1, s), la(t-1, s-1), [opt[s-1]] la(t-1, s-2))
    lb(F-1, s)  = 0 for s = S-1, and for s = S-2 iff S >= 2 and opt[S-1]; -inf otherwise
    lb(t, s)    = lse(lb(t+1, s) + e(t+1, s), lb(t+1, s+1) + e(t+1, s+1), [opt[s+1]] lb(t+1, s+2) + e(t+1, s+2))
    log_z       = lse over the end states of la(F-1, .)
    gamma(t, s) = exp(la + lb - log_z);  Gamma(t, c) = sum of gamma(t, s) over seq[s] = c;  occ(s) = sum_t gamma(t, s)
    infeasible: F == 0, S == 0 or log_z == -inf  (log_z = -inf, everything else zero)

fullsum_f64    the recurrences as written, float64, nothing shifted or scaled (float64 holds exp(-700))
brute_force    every admissible path of a tiny problem (align_ref.admissible_paths): log Z and gamma by enumeration
"""
from collections import namedtuple

import numpy as np

import align_ref as ar

FullSum = namedtuple('FullSum', 'log_z class_post state_post occ')
NEG = -np.inf


def lse(*xs):
    """Elementwise log(sum(exp(x))) of equally shaped float64 arrays; -inf where every term is -inf."""
    x = np.stack([np.asarray(v, dtype=np.float64) for v in xs])
    m = x.max(0)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide='ignore'):
        return np.where(np.isfinite(m), safe + np.log(np.exp(x - safe).sum(0)), NEG)


def _shift(v, n, fill=NEG):
    """v moved n places to the right (n > 0) or to the left (n < 0), ``fill`` coming in."""
    out = np.full_like(v, fill)
    if n > 0:
        out[n:] = v[:-n] if n < len(v) else []
    else:
        out[:n] = v[-n:] if -n < len(v) else []
    return out


def lattice(e, opt):
    """(la, lb, log_z) of e [F, S] float64 and opt [S]."""
    F, S = e.shape
    opt = np.asarray(opt).astype(bool)
    skip_in = np.zeros((S,), bool)                  # a skip INTO s: opt[s-1], s >= 2
    skip_in[2:] = opt[1:S - 1]
    skip_out = np.zeros((S,), bool)                 # a skip OUT OF s: opt[s+1], s + 2 < S
    skip_out[:max(S - 2, 0)] = opt[1:S - 1]
    la = np.full((F, S), NEG)
    la[0, 0] = e[0, 0]
    if S > 1 and opt[0]:
        la[0, 1] = e[0, 1]
    for t in range(1, F):
        p = la[t - 1]
        la[t] = e[t] + lse(p, _shift(p, 1), np.where(skip_in, _shift(p, 2), NEG))
    lb = np.full((F, S), NEG)
    lb[F - 1, S - 1] = 0.0
    if S > 1 and opt[S - 1]:
        lb[F - 1, S - 2] = 0.0
    for t in range(F - 2, -1, -1):
        g = lb[t + 1] + e[t + 1]
        lb[t] = lse(g, _shift(g, -1), np.where(skip_out, _shift(g, -2), NEG))
    log_z = float(lse(*(la[F - 1, s:s + 1] for s in range(S) if lb[F - 1, s] == 0.0))[0])
    return la, lb, log_z


def fullsum_f64(score, seq, opt=None, n_frames=None, n_seq=None):
    """One utterance.  score [F_max, C], seq [S_max]; outputs padded to F_max / S_max with zeros."""
    score = np.asarray(score, dtype=np.float64)
    F_max, C = score.shape
    seq = np.asarray(seq)
    S_max = len(seq)
    F = int(min(max(n_frames if n_frames is not None else F_max, 0), F_max))
    S = int(min(max(n_seq if n_seq is not None else S_max, 0), S_max))
    opt = np.zeros((S_max,), np.uint8) if opt is None else (np.asarray(opt) != 0).astype(np.uint8)
    none = FullSum(NEG, np.zeros((F_max, C)), np.zeros((F_max, S_max)), np.zeros((S_max,)))
    if F == 0 or S == 0:
        return none
    e = ar.emissions(score[:F], seq[:S], np.float64)
    la, lb, log_z = lattice(e, opt[:S])
    if log_z == NEG:
        return none
    with np.errstate(invalid='ignore'):
        ex = la + lb - log_z
    gamma = np.exp(np.where(np.isnan(ex), NEG, ex))                 # (-inf + -inf is -inf here, never a NaN)
    state_post = np.zeros((F_max, S_max))
    state_post[:F, :S] = gamma
    class_post = np.zeros((F_max, C))
    for s in range(S):
        if 0 <= seq[s] < C:
            class_post[:F, seq[s]] += gamma[:, s]
    return FullSum(log_z, class_post, state_post, state_post.sum(0))


def fullsum_batch_f64(score, seq, opt, n_frames, n_seq):
    """score [B, F_max, C], seq [B, S_max], opt [B, S_max] or None, lengths [B] -> FullSum of stacked arrays."""
    rows = [fullsum_f64(score[b], seq[b], None if opt is None else opt[b], int(n_frames[b]), int(n_seq[b])) for b in range(len(score))]
    return FullSum(*(np.stack([np.asarray(getattr(r, f), dtype=np.float64) for r in rows]) for f in FullSum._fields))


def brute_force(score, seq, opt=None):
    """(log Z, gamma [F, S]) over every admissible path, each path's emissions added in float64; (-inf, zeros) when no
    path has a finite score."""
    score = np.asarray(score, dtype=np.float64)
    F, S = score.shape[0], len(seq)
    opt = [0] * S if opt is None else list(opt)
    e = ar.emissions(score, seq, np.float64)
    paths = ar.admissible_paths(F, S, opt)
    w = np.array([sum(e[t, p[t]] for t in range(F)) for p in paths], dtype=np.float64)
    if not len(w) or w.max() == NEG:
        return NEG, np.zeros((F, S))
    m = w.max()
    pw = np.exp(w - m)
    log_z = m + np.log(pw.sum())
    gamma = np.zeros((F, S))
    for p, x in zip(paths, pw / pw.sum()):
        gamma[np.arange(F), p] += x
    return float(log_z), gamma
