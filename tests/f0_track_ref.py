"""Host reference of the pitch tracker with several candidates per frame (include/vc_hip.h, "Pitch tracking"; DESIGN.md
section 19).  It builds on f0_ref.py: frames, d and d' are f0_ref's, in float64 (the definition) or in the float32
restatement of the device's order of operations.

  candidates  lag tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) (+inf left of tau_min), d'(tau) <= d'(tau + 1) (+inf
              right of tau_max) and d'(tau) < ceiling; the n_cand of lowest d' (ties: the smaller lag), in ascending lag;
              f0 by f0_ref.refine, pitch = log2(f0), cost = d'(tau); n per frame; aperiodicity = min d' over the range
  viterbi     S = n_cand + 1 states (0 unvoiced, cost unvoiced_cost; k candidate k - 1; beyond n[f] absent), transition 0 /
              switch_cost / jump_cost * |pitch_i - pitch_j|; delta_f(j) = min_i (delta_{f-1}(i) + t(i, j)) + c_f(j), lowest
              i among equals; after every frame the minimum is subtracted and added into a float64 total; the last state
              is the lowest j of minimal delta.  ``dtype=np.float32`` follows the device operation for operation.

``weak_signal`` is the test signal with a weak, fluctuating fundamental under a strong second harmonic, on which YIN's
first dip below the threshold is often the one at half the period.
"""
import numpy as np

import f0_ref as fr


def dprime(x, sr=16000, hop=80, W=512, fmin=60.0, fmax=400.0, dtype=np.float64, block=256):
    """(d' [F, tau_max + 2] in ``dtype``, computed [F, tau_max + 2] bool).  ``computed`` is False where d' is SET, not
    calculated: lag 0 and every lag whose running sum is zero (exactly zero in either precision: all its terms are)."""
    tau_min, tau_max = fr.lag_range(sr, fmin, fmax)
    x = np.asarray(x, dtype=np.float32)
    F = fr.n_frames(len(x), hop)
    dp = np.empty((F, tau_max + 2), dtype)
    comp = np.empty((F, tau_max + 2), bool)
    for b0 in range(0, F, block):
        d = fr.difference(fr.frames(x, hop, W, tau_max, b0, b0 + block), W, tau_max, dtype)
        dp[b0:b0 + block] = fr.normalise(d, dtype)
        comp[b0:b0 + block] = fr.running_sum(d, dtype) > 0
    comp[:, 0] = False
    return dp, comp


def yin_from_dprime(dp, sr=16000, fmin=60.0, fmax=400.0, threshold=0.15, dtype=np.float64):
    """f0_ref.yin's (f0, aperiodicity) from a d' already computed (the same picks, the same parabola)."""
    tau_min, tau_max = fr.lag_range(sr, fmin, fmax)
    F = dp.shape[0]
    f0, ap = np.zeros(F, dtype), np.ones(F, dtype)
    for f in range(F):
        ap[f] = dp[f, tau_min:tau_max + 1].min()
        tau = fr.pick_lag(dp[f], tau_min, tau_max, dtype(threshold))
        if tau:
            f0[f] = fr.refine(dp[f], tau, sr, dtype)
    return f0, ap


def _flags(r, tol, ceiling, sign):
    """Local-minimum flags of r [F, L] with every comparison moved by sign * (the two values' tolerances)."""
    inf = np.full((r.shape[0], 1), np.inf)
    zero = np.zeros((r.shape[0], 1))
    left, tl = np.concatenate([inf, r[:, :-1]], 1), np.concatenate([zero, tol[:, :-1]], 1)
    right, tr = np.concatenate([r[:, 1:], inf], 1), np.concatenate([tol[:, 1:], zero], 1)
    with np.errstate(invalid='ignore'):
        return (r < left + sign * (tol + tl)) & (r <= right + sign * (tol + tr)) & (r < ceiling + sign * tol)


def select(dp, tau_min, tau_max, n_cand, ceiling):
    """(lags [F, n_cand] ascending, 0 beyond n; n [F]) of d' [F, tau_max + 2], any dtype."""
    r = dp[:, tau_min:tau_max + 1].astype(np.float64)
    key = np.where(_flags(r, np.zeros_like(r), float(ceiling), 0.0), r, np.inf)
    idx = np.argsort(key, axis=1, kind='stable')[:, :n_cand]                   # stable: the smaller lag wins a tie
    if idx.shape[1] < n_cand:
        idx = np.concatenate([idx, np.zeros((len(idx), n_cand - idx.shape[1]), idx.dtype)], 1)
        ok = np.zeros(idx.shape, bool)
        ok[:, :key.shape[1]] = np.isfinite(np.take_along_axis(key, idx[:, :key.shape[1]], 1))
    else:
        ok = np.isfinite(np.take_along_axis(key, idx, 1))
    lags = np.sort(np.where(ok, idx + tau_min, 1 << 30), axis=1)
    return np.where(lags < (1 << 30), lags, 0), ok.sum(1)


def marginal_frames(dp, comp, tau_min, tau_max, n_cand, ceiling, W):
    """Frames where one of the decisions -- a local-minimum flag, the ceiling, rank n_cand against rank n_cand + 1 --
    changes when every CALCULATED d' moves by a relative (W + tau_max) 2^-24 (f0_ref: the bound on float32's error in d');
    a d' that is set (1 where the running sum is zero) does not move.  A flag that can change counts only when its d'
    could be among the n_cand lowest."""
    delta = (W + tau_max) * 2.0 ** -24
    r = dp[:, tau_min:tau_max + 1].astype(np.float64)
    tol = np.where(comp[:, tau_min:tau_max + 1], delta * np.abs(r), 0.0)
    lenient, strict = _flags(r, tol, float(ceiling), 1.0), _flags(r, tol, float(ceiling), -1.0)
    sure = np.sort(np.where(strict, r, np.inf), axis=1)
    kth = sure[:, n_cand - 1] if sure.shape[1] >= n_cand else np.full(len(r), np.inf)
    unsure = (lenient & ~strict) & (r <= (kth * (1 + 2 * delta))[:, None])
    out = unsure.any(1)
    if sure.shape[1] > n_cand:
        a, b = sure[:, n_cand - 1], sure[:, n_cand]
        with np.errstate(invalid='ignore'):
            out |= np.isfinite(b) & (b - a <= delta * (a + b))
    return out


def candidates(x, sr=16000, hop=80, W=512, fmin=60.0, fmax=400.0, n_cand=8, ceiling=1.0, dtype=np.float64, dp=None):
    """dict(lag [F, n_cand] int (0 beyond n), f0, pitch, cost [F, n_cand] in ``dtype`` (0, 0, 1 beyond n), n [F],
    aperiodicity [F], marginal [F] bool (marginal_frames), dp, computed).  ``dp``: a (d', computed) pair already made."""
    tau_min, tau_max = fr.lag_range(sr, fmin, fmax)
    dp, comp = dprime(x, sr, hop, W, fmin, fmax, dtype) if dp is None else dp
    lags, n = select(dp, tau_min, tau_max, n_cand, dtype(ceiling))
    F = dp.shape[0]
    f0, cost = np.zeros((F, n_cand), dtype), np.ones((F, n_cand), dtype)
    for f in range(F):
        for k in range(n[f]):
            f0[f, k] = fr.refine(dp[f], int(lags[f, k]), sr, dtype)
            cost[f, k] = dp[f, lags[f, k]]
    pitch = np.where(f0 > 0, np.log2(np.where(f0 > 0, f0, 1)), 0).astype(dtype)
    return dict(lag=lags, f0=f0, pitch=pitch, cost=cost, n=n.astype(np.int64), aperiodicity=dp[:, tau_min:tau_max + 1].min(1),
                marginal=marginal_frames(dp, comp, tau_min, tau_max, n_cand, ceiling, W), dp=dp, computed=comp)


def viterbi(pitch, cost, n, unvoiced_cost=0.15, jump_cost=0.5, switch_cost=0.1, dtype=np.float64, details=False):
    """(state [F] int, total) of one utterance's lattice: pitch, cost [F, n_cand], n [F].  total is float64 whatever the
    dtype (the per-frame minima are added in float64).  With details also marginal [F] bool: a frame where, for some
    state, the two best predecessors (or, at the last frame, the two best states) are closer than the float32 spacing
    at the largest value of that frame's sums -- there a float32 recurrence may choose the other one."""
    pitch, cost, n = np.asarray(pitch), np.asarray(cost), np.asarray(n)
    F, nc = pitch.shape
    S = nc + 1
    n = np.clip(n, 0, nc)
    here = np.arange(S)[None, :] <= n[:, None]
    p = np.zeros((F, S), dtype)
    p[:, 1:] = pitch
    p[~here] = 0
    c = np.full((F, S), np.inf, dtype)
    c[:, 0] = dtype(unvoiced_cost)
    c[:, 1:] = cost
    c[~here] = np.inf
    uv = np.zeros((S, S), bool)
    uv[0, :] = uv[:, 0] = True
    sw = np.full((S, S), dtype(switch_cost), dtype)
    sw[0, 0] = 0
    jc = dtype(jump_cost)
    bp = np.zeros((F, S), np.int64)
    marginal = np.zeros(F, bool)
    cols = np.arange(S)
    total = np.float64(0)
    delta = c[0].copy()
    for f in range(F):
        if f:
            t = np.where(uv, sw, jc * np.abs(p[f - 1][:, None] - p[f][None, :]))
            cand = delta[:, None] + t
            bp[f] = np.argmin(cand, axis=0)                                     # the lowest i among equals
            delta = cand[bp[f], cols] + c[f]
            if details:
                two = np.sort(cand, axis=0)[:2] if S > 1 else None
                fin = cand[np.isfinite(cand)]
                eps = float(np.spacing(np.float32(max(float(fin.max()), float(c[f][here[f]].max())))))
                marginal[f] = bool(((two[1] - two[0])[here[f]] < eps).any())
        m = delta.min()
        delta = delta - m
        total += np.float64(m)
    state = np.zeros(F, np.int64)
    if F:
        state[F - 1] = int(np.argmin(delta))
        if details:
            two = np.sort(delta)[:2]
            marginal[F - 1] |= bool(len(two) > 1 and two[1] - two[0] < float(np.spacing(np.float32(1.0))))
        for f in range(F - 1, 0, -1):
            state[f - 1] = bp[f, state[f]]
    return (state, total, marginal) if details else (state, total)


def track(x, sr=16000, hop=80, W=512, fmin=60.0, fmax=400.0, threshold=0.15, jump_cost=0.5, switch_cost=0.1, n_cand=8,
          ceiling=1.0, dtype=np.float64, cand=None):
    """(f0 [F], state [F], total, candidates dict): candidates, then viterbi with unvoiced_cost = threshold."""
    cand = candidates(x, sr, hop, W, fmin, fmax, n_cand, ceiling, dtype) if cand is None else cand
    state, total = viterbi(cand['pitch'], cand['cost'], cand['n'], threshold, jump_cost, switch_cost, dtype)
    f0 = np.where(state > 0, cand['f0'][np.arange(len(state)), np.maximum(state, 1) - 1], 0).astype(dtype)
    return f0, state, total, cand


def weak_signal(seed, seconds=2.0, sr=16000):
    """(x float32 [n], f0_true float64 [n], voiced bool [n]): a gliding fundamental whose own amplitude a(t) swings
    between 0.03 and 0.53 under a second and a fourth harmonic of fixed amplitude, noise of sigma 0.02; three gaps of
    0.12 s at three of the eight tenths of the signal (the first silence, the other two noise of sigma 0.05)."""
    rng = np.random.RandomState(seed)
    n = int(round(seconds * sr))
    t = np.arange(n) / float(sr)
    f0 = rng.uniform(90.0, 200.0) * 2.0 ** (0.35 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t))
    ph = 2.0 * np.pi * np.cumsum(f0) / sr
    a = 0.03 + 0.25 * (1.0 + np.sin(2 * np.pi * rng.uniform(1.5, 3.0) * t + rng.uniform(0.0, 6.0)))
    x = 0.2 * (a * np.sin(ph) + np.sin(2 * ph + 0.3) + 0.5 * a * np.sin(3 * ph + 1.0) + 0.4 * np.sin(4 * ph + 2.0))
    x = x + 0.02 * rng.standard_normal(n)
    voiced = np.ones(n, bool)
    g = int(0.12 * sr)
    for k, slot in enumerate(rng.permutation(np.arange(1, 9))[:3]):
        s = int(slot * n / 10)
        x[s:s + g] = 0.0 if k == 0 else 0.05 * rng.standard_normal(g)
        voiced[s:s + g] = False
    return x.astype(np.float32), f0, voiced


def gross_errors(f0, f0_true, voiced, hop=80, W=512, sr=16000, fmin=60.0, cents=300.0):
    """(gross, scored): frames of f0_ref.fully_voiced_frames more than ``cents`` from the truth at the frame's centre
    (an unvoiced frame there counts as gross)."""
    tau_max = fr.lag_range(sr, fmin)[1]
    keep = fr.fully_voiced_frames(voiced, hop, W, tau_max)
    centre = np.clip(np.arange(len(keep)) * hop, 0, len(f0_true) - 1)
    got, want = np.asarray(f0, np.float64)[:len(keep)][keep], f0_true[centre][keep]
    bad = got <= 0
    with np.errstate(divide='ignore'):
        bad |= np.abs(1200.0 * np.log2(np.where(got > 0, got, 1.0) / want)) > cents
    return int(bad.sum()), int(keep.sum())


def dyadic_lattice(rng, F, n_cand, p_empty=0.1):
    """A lattice on which every float32 sum of the recurrence is exact: (pitch, cost [F, n_cand] float32, multiples of
    1/64 in [0, 2]; n [F] in [0, n_cand], about ``p_empty`` of the frames with n = 0).  Slots beyond n hold values too
    (cheap ones: a kernel that read them would take them).  With the three parameters multiples of 1/16 every product is
    a multiple of 1/1024 below 4 and every sum a multiple of 1/1024 below 16: 14 bits."""
    pitch = (rng.randint(0, 129, (F, n_cand)) / 64.0).astype(np.float32)
    cost = (rng.randint(0, 129, (F, n_cand)) / 64.0).astype(np.float32)
    n = rng.randint(0, n_cand + 1, F)
    n[rng.uniform(size=F) < p_empty] = 0
    beyond = np.arange(n_cand)[None, :] >= n[:, None]
    cost[beyond] = 0.0
    return pitch, cost, n.astype(np.int32)
