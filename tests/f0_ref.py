"""Host reference of the F0 tracker and the F0 / voicing figures (include/vc_hip.h, "Evaluation").

YIN (de Cheveigne and Kawahara 2002), steps 2 to 5, on the raw waveform:

  frames      F = 1 + len // hop; frame f reads x[s .. s + W + tau_max], s = f * hop - (W + tau_max) // 2, zeros outside
  difference  d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2, tau = 0 .. tau_max + 1, the DIRECT form, j ascending
  normalised  d'(0) = 1, d'(tau) = d(tau) * tau / sum_{k = 1..tau} d(k), and 1 where that sum is zero
  pick        the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then on while tau + 1 <= tau_max and
              d'(tau + 1) < d'(tau); none: unvoiced, f0 = 0
  refine      offset = 0.5 (y0 - y2) / (y0 - 2 y1 + y2) through d'(tau - 1 .. tau + 1) when the denominator is positive,
              else 0, clamped to [-0.5, 0.5]; f0 = sr / (tau + offset)
  aperiodicity  min over [tau_min, tau_max] of d', voiced or not

``yin(..., dtype=np.float64)`` is the definition.  ``dtype=np.float32`` is the restatement in the device's working
precision and order of operations: one fused multiply-add chain per lag (a float64 product of two float32 values is
exact, so rounding acc + df * df once from float64 restates the fused operation), the running sum over lags as the
kernel's scan (Kogge-Stone inside groups of 64 lags, then the group totals added in order), one rounded product and one
correctly rounded division per d', the pick and the parabola in float32.

``metrics`` are the float64 figures of a pair of tracks along a path; ``dtype=np.float32`` restates them in float32.
``glide_signal`` is the test signal of the issue's measurement (seeded): five harmonics of a gliding fundamental, slow
amplitude modulation, two gaps of silence and two of white noise, noise of sigma 0.02 on the voiced parts.
"""
import math

import numpy as np

MARGIN = 1e-3               # a decision within this of the threshold may fall either way in float32


def lag_range(sr, fmin=60.0, fmax=400.0):
    return int(math.floor(sr / fmax)), int(math.ceil(sr / fmin))


def n_frames(length, hop):
    return 1 + int(length) // int(hop)


def frames(x, hop, W, tau_max, f0=0, f1=None):
    """Rows f0 .. f1-1 of the [F, W + tau_max + 1] matrix of frames, zeros outside the signal."""
    x = np.asarray(x)
    F = n_frames(len(x), hop)
    f1 = F if f1 is None else min(f1, F)
    span = W + tau_max + 1
    idx = (np.arange(f0, f1) * hop - (W + tau_max) // 2)[:, None] + np.arange(span)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    src = x if len(x) else np.zeros(1, x.dtype)                       # an empty utterance: one frame of zeros
    return np.where(ok, src[np.clip(idx, 0, len(src) - 1)], 0).astype(x.dtype)


def difference(fr, W, tau_max, dtype=np.float64):
    """d [F, tau_max + 2] of a block of frames, the direct form, j ascending."""
    n = tau_max + 2
    fr = fr.astype(dtype)
    acc = np.zeros((fr.shape[0], n), dtype)
    for j in range(W):
        df = fr[:, j:j + 1] - fr[:, j:j + n]
        if dtype == np.float32:
            acc = (acc.astype(np.float64) + df.astype(np.float64) ** 2).astype(np.float32)       # fmaf(df, df, acc)
        else:
            acc += df * df
    return acc


def running_sum(d, dtype=np.float64):
    """sum_{k <= tau} d(k) (d(0) is zero).  float32: the kernel's scan."""
    if dtype != np.float32:
        return np.cumsum(d, axis=1)
    F, n = d.shape
    nw = -(-n // 64)
    v = np.zeros((F, nw * 64), np.float32)
    v[:, :n] = d
    v = v.reshape(F, nw, 64)
    for s in (1, 2, 4, 8, 16, 32):
        u = v.copy()
        u[:, :, s:] = v[:, :, s:] + v[:, :, :-s]
        v = u
    off = np.zeros((F, nw), np.float32)
    for w in range(1, nw):
        off[:, w] = off[:, w - 1] + v[:, w - 1, 63]
    return (v + off[:, :, None]).reshape(F, nw * 64)[:, :n]


def normalise(d, dtype=np.float64):
    S = running_sum(d, dtype)
    tau = np.arange(d.shape[1]).astype(dtype)[None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        dp = (d * tau) / S
    dp = np.where(S > 0, dp, dtype(1))
    dp[:, 0] = 1
    return dp.astype(dtype)


def pick_lag(dp, tau_min, tau_max, threshold):
    """The lag of one frame's d' (0: unvoiced)."""
    below = np.nonzero(dp[tau_min:tau_max + 1] < threshold)[0]
    if below.size == 0:
        return 0
    tau = tau_min + int(below[0])
    while tau + 1 <= tau_max and dp[tau + 1] < dp[tau]:
        tau += 1
    return tau


def refine(dp, tau, sr, dtype=np.float64):
    y0, y1, y2 = dtype(dp[tau - 1]), dtype(dp[tau]), dtype(dp[tau + 1])
    den = (y0 - dtype(2) * y1) + y2
    off = dtype(0.5) * (y0 - y2) / den if den > 0 else dtype(0)
    off = min(max(off, dtype(-0.5)), dtype(0.5))
    return dtype(sr) / (dtype(tau) + off)


def yin(x, sr=16000, hop=80, W=512, fmin=60.0, fmax=400.0, threshold=0.15, dtype=np.float64, details=False, block=256,
        tau_min=None, tau_max=None):
    """(f0 [F], aperiodicity [F]) in ``dtype``; with details also a dict: tau [F] (0 unvoiced), marginal [F] (bool: the
    voicing decision or the choice of the dip changes when the threshold moves by MARGIN either way), floor_cents [F],
    floor_ap [F] (what a relative error of (W + tau_max) 2^-24 in every d' can move the result by; see
    tests/test_f0_gpu.py).  ``tau_min`` / ``tau_max``: the lag range itself, in place of the one fmin and fmax give."""
    if tau_min is None or tau_max is None:
        tau_min, tau_max = lag_range(sr, fmin, fmax)
    x = np.asarray(x, dtype=np.float32)                                # the samples are float32 on either side
    F = n_frames(len(x), hop)
    f0, ap = np.zeros(F, dtype), np.ones(F, dtype)
    taus, marginal = np.zeros(F, np.int64), np.zeros(F, bool)
    floor_c, floor_a = np.zeros(F), np.zeros(F)
    thr = dtype(threshold)
    delta = (W + tau_max) * 2.0 ** -24
    for b0 in range(0, F, block):
        dp = normalise(difference(frames(x, hop, W, tau_max, b0, b0 + block), W, tau_max, dtype), dtype)
        for r in range(dp.shape[0]):
            f, row = b0 + r, dp[r]
            ap[f] = row[tau_min:tau_max + 1].min()
            tau = pick_lag(row, tau_min, tau_max, thr)
            taus[f] = tau
            if tau:
                f0[f] = refine(row, tau, sr, dtype)
            if details:
                lo, hi = pick_lag(row, tau_min, tau_max, thr - dtype(MARGIN)), pick_lag(row, tau_min, tau_max, thr + dtype(MARGIN))
                marginal[f] = abs(float(ap[f]) - float(thr)) < MARGIN or lo != tau or hi != tau
                floor_a[f] = delta * float(ap[f])
                if tau:
                    y0, y1, y2 = (float(v) for v in row[tau - 1:tau + 2])
                    den = y0 - 2 * y1 + y2
                    off = min(max(0.5 * (y0 - y2) / den, -0.5), 0.5) if den > 0 else 0.0
                    d_off = delta * max(y0, y1, y2) * (1 + 4 * abs(off)) / den if den > 0 else 0.0
                    floor_c[f] = 1200.0 / math.log(2.0) * d_off / (tau + off)
    if details:
        return f0, ap, dict(tau=taus, marginal=marginal, floor_cents=floor_c, floor_ap=floor_a)
    return f0, ap


def dprime(x, hop, W, tau_max, dtype=np.float64, block=256):
    """(d' [F, tau_max + 2] in ``dtype``, computed [F, tau_max + 2] bool: False where d' is set, not calculated -- lag 0
    and every lag whose running sum is zero) for any hop, W and tau_max."""
    x = np.asarray(x, dtype=np.float32)
    F = n_frames(len(x), hop)
    dp, comp = np.empty((F, tau_max + 2), dtype), np.empty((F, tau_max + 2), bool)
    for b0 in range(0, F, block):
        d = difference(frames(x, hop, W, tau_max, b0, b0 + block), W, tau_max, dtype)
        dp[b0:b0 + block] = normalise(d, dtype)
        comp[b0:b0 + block] = running_sum(d, dtype) > 0
    comp[:, 0] = False
    return dp, comp


def candidates(x, sr, hop, W, tau_min, tau_max, n_cand, ceiling, dtype=np.float64):
    """The candidates of include/vc_hip.h, "Pitch tracking", for any configuration: f0_track_ref's selection and its
    marginal frames on this module's d'.  dict(lag [F, n_cand] (0 beyond n), f0, pitch, cost (0, 0, 1 beyond n), n [F],
    aperiodicity [F], marginal [F], dp)."""
    import f0_track_ref as tr                                          # (it imports this module)
    dp, comp = dprime(x, hop, W, tau_max, dtype)
    lags, n = tr.select(dp, tau_min, tau_max, n_cand, dtype(ceiling))
    F = dp.shape[0]
    f0, cost = np.zeros((F, n_cand), dtype), np.ones((F, n_cand), dtype)
    for f in range(F):
        for k in range(n[f]):
            f0[f, k] = refine(dp[f], int(lags[f, k]), sr, dtype)
            cost[f, k] = dp[f, lags[f, k]]
    pitch = np.where(f0 > 0, np.log2(np.where(f0 > 0, f0, 1)), 0).astype(dtype)
    return dict(lag=lags, f0=f0, pitch=pitch, cost=cost, n=n.astype(np.int64), aperiodicity=dp[:, tau_min:tau_max + 1].min(1),
                marginal=tr.marginal_frames(dp, comp, tau_min, tau_max, n_cand, ceiling, W), dp=dp)


def cents(fa, fb):
    return 1200.0 * np.log2(np.asarray(fa, np.float64) / np.asarray(fb, np.float64))


def metrics(f0_a, f0_b, len_a, len_b, path=None, dtype=np.float64):
    """The figures of one pair: dict(n_cells, n_both_voiced, n_vuv_mismatch, vuv_error, f0_rmse_cents, f0_rmse_hz,
    logf0_corr).  path: [n, 2] cells (i, j), or None for (i, i), i < min(len_a, len_b).  A cell outside
    [0, len_a) x [0, len_b) is skipped and not counted.  vuv_error is NaN without a cell; the RMSE values are NaN
    without a both-voiced cell; the correlation is NaN with fewer than two both-voiced cells or when one side's f0 is
    the same in all of them (zero variance)."""
    fa, fb = np.asarray(f0_a)[:len_a].astype(dtype), np.asarray(f0_b)[:len_b].astype(dtype)
    if path is None:
        n = min(len_a, len_b)
        i = j = np.arange(n)
    else:
        p = np.asarray(path, dtype=np.int64).reshape(-1, 2)
        ok = (p[:, 0] >= 0) & (p[:, 0] < len_a) & (p[:, 1] >= 0) & (p[:, 1] < len_b)
        i, j = p[ok, 0], p[ok, 1]
    a, b = fa[i], fb[j]
    va, vb = a > 0, b > 0
    both = va & vb
    nan = dtype(np.nan)
    out = dict(n_cells=int(len(i)), n_both_voiced=int(both.sum()), n_vuv_mismatch=int((va ^ vb).sum()))
    out['vuv_error'] = dtype(out['n_vuv_mismatch']) / dtype(out['n_cells']) if out['n_cells'] else nan
    a, b = a[both], b[both]
    n = dtype(len(a))
    if len(a) == 0:
        out.update(f0_rmse_cents=nan, f0_rmse_hz=nan, logf0_corr=nan)
        return out
    c = dtype(1200) * np.log2(a / b)
    out['f0_rmse_cents'] = np.sqrt((c * c).sum(dtype=dtype) / n)
    out['f0_rmse_hz'] = np.sqrt(((a - b) ** 2).sum(dtype=dtype) / n)
    if len(a) < 2 or a.min() == a.max() or b.min() == b.max():
        out['logf0_corr'] = nan
    else:
        la, lb = np.log2(a), np.log2(b)
        la, lb = la - la.sum(dtype=dtype) / n, lb - lb.sum(dtype=dtype) / n
        out['logf0_corr'] = (la * lb).sum(dtype=dtype) / np.sqrt((la * la).sum(dtype=dtype) * (lb * lb).sum(dtype=dtype))
    return out


def harmonic_tone(f0_track, sr=16000, n_harm=5):
    """Five harmonics (amplitudes 1 / h) of a fundamental given per sample; float64, peak below 2.3."""
    ph = 2.0 * np.pi * np.cumsum(np.asarray(f0_track, np.float64)) / sr
    return sum(np.sin(h * ph) / h for h in range(1, n_harm + 1))


def glide_signal(seed, seconds=2.0, sr=16000, pitch=1.0, stretch=1.0):
    """The test signal: returns (x float32 [n], f0_true float64 [n], voiced bool [n]).  ``pitch`` multiplies the
    fundamental and ``stretch`` the duration (the same utterance said higher and slower: the glide, the modulation and
    the gaps stretch along).
    f0 = U(90, 220) * 2^(0.35 sin(2 pi U(0.5, 1.5) t)), five harmonics, amplitude 0.3 * (1 + 0.3 sin(2 pi U(2, 5) t)),
    noise of sigma 0.02 on the voiced parts; two gaps of silence and two of white noise (sigma 0.1), each 0.12 s, at
    seeded places that do not overlap."""
    rng = np.random.RandomState(seed)
    n = int(round(seconds * stretch * sr))
    t = np.arange(n) / float(sr) / stretch
    base, rate, am = rng.uniform(90.0, 220.0), rng.uniform(0.5, 1.5), rng.uniform(2.0, 5.0)
    f0 = pitch * base * 2.0 ** (0.35 * np.sin(2 * np.pi * rate * t))
    x = 0.3 * (1.0 + 0.3 * np.sin(2 * np.pi * am * t)) * harmonic_tone(f0, sr) + 0.02 * rng.standard_normal(n)
    voiced = np.ones(n, bool)
    g = int(0.12 * stretch * sr)
    slots = rng.permutation(np.arange(1, 9))[:4]                          # four of eight places, 0.2 s apart
    for k, slot in enumerate(slots):
        s = int(slot * n / 10)
        x[s:s + g] = 0.0 if k < 2 else 0.1 * rng.standard_normal(g)
        voiced[s:s + g] = False
    return x.astype(np.float32), f0, voiced


def fully_voiced_frames(voiced, hop, W, tau_max):
    """Frames whose whole span [s, s + W + tau_max] lies inside the signal and is voiced."""
    F = n_frames(len(voiced), hop)
    bad = np.concatenate([[0], np.cumsum(~voiced)])
    s = np.arange(F) * hop - (W + tau_max) // 2
    e = s + W + tau_max + 1
    inside = (s >= 0) & (e <= len(voiced))
    return inside & (bad[np.clip(e, 0, len(voiced))] - bad[np.clip(s, 0, len(voiced))] == 0)
