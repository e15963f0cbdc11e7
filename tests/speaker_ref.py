"""The speaker-similarity definitions of include/vc_hip.h ("Speaker") restated in numpy: features, the mixture's per-frame
log-likelihood, the score figures, the E-step statistics, the EM and MAP updates, the deterministic initialisation and the
fit.  float64 by default; ``dtype=np.float32`` runs the same formulas with every intermediate rounded to float32 -- the
control that says what float32 arithmetic alone costs, against which the tolerances of the device tests are set.  The
statistics N, S1, S2, L are float64 in both (the device accumulates them in float64)."""
import numpy as np

LOG_2PI = np.log(2.0 * np.pi)
W_FLOOR = 2.0 ** -40


# ---------------------------------------------------------------------------------------------------------------- features
def features(cep, length, mask=None, deltas=True, cmn=True, dtype=np.float64):
    """cep [F, n_coef] -> [F, D]; rows from ``length`` on are zeros; the mean over the kept frames (mask set, t < length) is
    subtracted with cmn; without a kept frame nothing is subtracted."""
    cep = np.asarray(cep)
    F, n_coef = cep.shape
    c = cep[:length].astype(dtype)
    cols = [c]
    if deltas:
        idx = lambda k: np.clip(np.arange(length) + k, 0, max(length - 1, 0))
        d1 = c[idx(1)] - c[idx(-1)]
        d2 = c[idx(2)] - c[idx(-2)]
        cols.append(((d1 + dtype(2) * d2) / dtype(10)).astype(dtype))
    f = np.concatenate(cols, 1) if length else np.zeros((0, n_coef * (2 if deltas else 1)), dtype)
    if cmn and length:
        keep = np.ones(length, bool) if mask is None else np.asarray(mask[:length]).astype(bool)
        if keep.any():
            mean = (f[keep].astype(np.float64).sum(0) / keep.sum()).astype(dtype)
            f = (f - mean).astype(dtype)
    out = np.zeros((F, f.shape[1]), dtype)
    out[:length] = f
    return out


def _delta_f32(c, length):
    """The delta columns as the device forms them: two rounded differences, one fused multiply-add (formed in float64, where
    2 d2 + d1 of two float32 is exact unless their exponents lie more than 29 apart, and rounded once), one correctly rounded
    division."""
    idx = lambda k: np.clip(np.arange(length) + k, 0, max(length - 1, 0))
    d1 = (c[idx(1)] - c[idx(-1)]).astype(np.float32)
    d2 = (c[idx(2)] - c[idx(-2)]).astype(np.float32)
    return ((2.0 * d2.astype(np.float64) + d1.astype(np.float64)).astype(np.float32) / np.float32(10)).astype(np.float32)


def features_f32(cep, length, mask=None, deltas=True, cmn=True):
    """features() in float32 with the device's operation order: the column sums of the kept frames in float64, lane r of
    four adding the kept frames r, r + 4, ... ascending, the partial sums added as ((0 + 1) + 2) + 3, the quotient rounded
    to float32 once, one rounded subtraction.  ``length`` is clamped to [0, F] as the launch clamps it."""
    cep = np.asarray(cep, np.float32)
    F, n_coef = cep.shape
    length = min(max(int(length), 0), F)
    D = n_coef * (2 if deltas else 1)
    out = np.zeros((F, D), np.float32)
    if not length:
        return out
    c = cep[:length]
    f = np.concatenate([c, _delta_f32(c, length)], 1) if deltas else c.copy()
    if cmn:
        keep = np.ones(length, bool) if mask is None else np.asarray(mask[:length]).astype(bool)
        part = np.zeros((4, D))
        for r in range(4):
            for t in np.nonzero(keep[r::4])[0]:
                part[r] += f[r + 4 * t].astype(np.float64)
        if keep.any():
            mean = ((((part[0] + part[1]) + part[2]) + part[3]) / float(keep.sum())).astype(np.float32)
            f = (f - mean).astype(np.float32)
    out[:length] = f
    return out


# ------------------------------------------------------------------------------------------------------------------- model
def log_norm(w, var):
    """c_m = log w_m - 0.5 sum_d log(2 pi var_md), float64."""
    return np.log(np.asarray(w, np.float64)) - 0.5 * (LOG_2PI + np.log(np.asarray(var, np.float64))).sum(1)


def component_loglik(x, w, mu, var, dtype=np.float64):
    """l [n, M] and q [n, M] = sum_d (x - mu)^2 / var, the sum over d ascending."""
    x, mu = np.asarray(x).astype(dtype), np.asarray(mu).astype(dtype)
    c = log_norm(w, var).astype(dtype)
    iv = (1.0 / np.asarray(var, np.float64)).astype(dtype)
    q = np.zeros((x.shape[0], mu.shape[0]), dtype)
    for d in range(x.shape[1]):
        df = (x[:, d, None] - mu[None, :, d]).astype(dtype)
        q = (q + ((df * df).astype(dtype) * iv[None, :, d]).astype(dtype)).astype(dtype)
    return (c[None] - dtype(0.5) * q).astype(dtype), q


def loglik(x, w, mu, var, dtype=np.float64):
    """ll [n] = max_m l_m + log sum_m exp(l_m - max), and the running-error quantity E [n] = |c_m*| + q_m* / 2 of the
    dominant component m* (taken from the float64 run by the callers)."""
    l, q = component_loglik(x, w, mu, var, dtype)
    top = l.argmax(1)
    mx = l.max(1)
    ll = (mx + np.log(np.exp((l - mx[:, None]).astype(dtype)).astype(dtype).sum(1, dtype=dtype)).astype(dtype)).astype(dtype)
    c = log_norm(w, var)
    rows = np.arange(len(top))
    E = np.abs(c[top]) + 0.5 * q[rows, top].astype(np.float64)
    return ll, E


def frame_bound(D, M, E):
    """|ll_device - ll_float64| <= (D + log2 M + 16) 2^-24 E: the forward bound of a D-term fused sum and a log-sum-exp."""
    return (D + np.log2(M) + 16.0) * 2.0 ** -24 * np.asarray(E, np.float64)


def score(ll_a, ll_b, length, mask=None):
    """(n_frames, mean ll_a, mean ll_b, llr) over the kept frames; NaN figures without one."""
    keep = np.zeros(len(ll_a), bool)
    keep[:length] = True
    if mask is not None:
        keep &= np.asarray(mask).astype(bool)
    n = int(keep.sum())
    if n == 0:
        return 0, np.nan, np.nan, np.nan
    a = np.asarray(ll_a, np.float64)[keep].sum() / n
    b = np.asarray(ll_b, np.float64)[keep].sum() / n
    return n, a, b, a - b


def accumulate(x, lens, groups, n_groups, w, mu, var, masks=None, dtype=np.float64, ll=None):
    """x [B, F, D].  Returns dict N [G, M], S1, S2 [G, M, D], L [G] (float64) and A1 = sum gamma |x|, the right-hand side of the
    S1 bound (that of S2 is S2 itself, that of N is N).  ll [B, F]: the stored log-likelihoods gamma is normalised by (the
    device's own, for a like-for-like control); None: this function's."""
    B, F, D = x.shape
    M = len(w)
    out = dict(N=np.zeros((n_groups, M)), S1=np.zeros((n_groups, M, D)), S2=np.zeros((n_groups, M, D)), L=np.zeros(n_groups),
               A1=np.zeros((n_groups, M, D)))
    for b in range(B):
        g = int(groups[b])
        if not 0 <= g < n_groups:
            continue
        keep = np.zeros(F, bool)
        keep[:lens[b]] = True
        if masks is not None:
            keep &= np.asarray(masks[b]).astype(bool)
        if not keep.any():
            continue
        xb = np.asarray(x[b])[keep]
        l, _ = component_loglik(xb, w, mu, var, dtype)
        llb = loglik(xb, w, mu, var, dtype)[0] if ll is None else np.asarray(ll[b])[keep].astype(dtype)
        gam = np.exp((l - llb[:, None]).astype(dtype)).astype(dtype).astype(np.float64)
        x64 = xb.astype(np.float64)
        out['N'][g] += gam.sum(0)
        out['S1'][g] += gam.T @ x64
        out['S2'][g] += gam.T @ (x64 * x64)
        out['A1'][g] += gam.T @ np.abs(x64)
        out['L'][g] += llb.astype(np.float64).sum()
    return out


def update_em(N, S1, S2, mu_old, var_old, var_floor, min_count=1.0):
    """(w, mu, var) as float32 from float64 statistics of ONE group; float64 arithmetic, each output rounded once."""
    N, S1, S2 = np.asarray(N, np.float64), np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    with np.errstate(all='ignore'):
        wv = N / N.sum()
        w = np.where(wv > W_FLOOR, wv, W_FLOOR)
        mean = S1 / N[:, None]
        v = S2 / N[:, None] - mean * mean
    v = np.where(v > np.asarray(var_floor, np.float64)[None], v, np.asarray(var_floor, np.float64)[None])
    old = N < np.float64(np.float32(min_count))
    mu = np.where(old[:, None], np.asarray(mu_old, np.float32), mean.astype(np.float32))
    var = np.where(old[:, None], np.asarray(var_old, np.float32), v.astype(np.float32))
    return w.astype(np.float32), mu.astype(np.float32), var.astype(np.float32)


def update_map(N, S1, mu_ubm, relevance=16.0):
    """means [G, M, D] float32: alpha = N / (N + r); mu = alpha S1 / N + (1 - alpha) mu_ubm; N = 0 gives mu_ubm exactly."""
    N, S1 = np.asarray(N, np.float64), np.asarray(S1, np.float64)
    ubm = np.asarray(mu_ubm, np.float32)
    r = np.float64(np.float32(relevance))
    with np.errstate(all='ignore'):
        alpha = (N / (N + r))[..., None]
        mu = alpha * (S1 / N[..., None]) + (1.0 - alpha) * ubm.astype(np.float64)[None]
    return np.where((N > 0)[..., None], mu.astype(np.float32), ubm[None]).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- fit
def init_rows(lens, n_components):
    """(utterance, frame) of the initial means: positions floor((m + 1/2) n / M) of the concatenation of all frames below
    lens."""
    lens = np.asarray(lens, np.int64)
    n = int(lens.sum())
    pos = ((2 * np.arange(n_components, dtype=np.int64) + 1) * n) // (2 * n_components)
    ends = np.cumsum(lens)
    b = np.searchsorted(ends, pos, side='right')
    return b, pos - (ends[b] - lens[b])


def global_variance(x, lens, masks=None):
    """(variance of the kept frames per dimension, their count), as one E-step with a single component gives them (float64
    statistics, the variance rounded to float32 once)."""
    B, F, D = x.shape
    st = accumulate(x, lens, np.zeros(B, int), 1, np.ones(1), np.zeros((1, D)), np.ones((1, D)), masks)
    mean = st['S1'][0, 0] / st['N'][0, 0]
    return (st['S2'][0, 0] / st['N'][0, 0] - mean * mean).astype(np.float32), st['N'][0, 0]


def fit(x, lens, n_components=64, n_iter=10, masks=None, var_floor=0.01, min_count=1.0, dtype=np.float64, init=None):
    """(w, mu, var, trace): trace[i] = the mean ll per kept frame before update i.  init = (w, mu, var) overrides the
    deterministic initialisation (the device's own, for a like-for-like trace)."""
    B, F, D = x.shape
    gv, n_kept = global_variance(x, lens, masks)
    if init is None:
        b, f = init_rows(lens, n_components)
        mu = np.asarray(x)[b, f].astype(np.float32)
        var = np.tile(gv[None], (n_components, 1)).astype(np.float32)
        w = np.full(n_components, np.float32(1.0 / n_components), np.float32)
    else:
        w, mu, var = (np.asarray(a, np.float32) for a in init)
    floor = (np.float32(var_floor) * gv).astype(np.float32)
    trace = []
    for _ in range(n_iter):
        st = accumulate(x, lens, np.zeros(B, int), 1, w, mu, var, masks, dtype)
        trace.append(st['L'][0] / n_kept)
        w, mu, var = update_em(st['N'][0], st['S1'][0], st['S2'][0], mu, var, floor, min_count)
    return w, mu, var, np.array(trace)


# ----------------------------------------------------------------------------------------------------------- synthetic set
def synthetic_speakers(seed=11, n_speakers=4, n_utt=6, D=8, n_mix=4, lo=150, hi=400):
    """4 "speakers", each a random 4-component mixture in D = 8 whose means lie at unit spread around a shared centre; 6
    utterances of 150 - 400 frames each.  Returns x [B, Fmax, D] float32 (zeros beyond the length), lens [B], speaker [B]."""
    rng = np.random.RandomState(seed)
    centre = rng.standard_normal(D)
    utts, lens, spk = [], [], []
    for s in range(n_speakers):
        means = centre + rng.standard_normal((n_mix, D))
        std = 0.3 + 0.3 * rng.rand(n_mix, D)
        pw = rng.dirichlet(np.full(n_mix, 4.0))
        for _ in range(n_utt):
            n = int(rng.randint(lo, hi + 1))
            k = rng.choice(n_mix, n, p=pw)
            utts.append((means[k] + std[k] * rng.standard_normal((n, D))).astype(np.float32))
            lens.append(n)
            spk.append(s)
    x = np.zeros((len(utts), max(lens), D), np.float32)
    for b, u in enumerate(utts):
        x[b, :len(u)] = u
    return x, np.array(lens), np.array(spk)
