"""The postfilters of include/vc_hip.h ("Postfilters") restated in numpy: trajectory statistics, the global-variance
filter, the modulation-spectrum statistics and the modulation-spectrum filter.  Every function takes ``dtype``: float64 is the
reference, float32 its twin -- the same definition with every operation in float32, the transforms as plain 64-term
float32 matrix products (another summation and transform order than the device's, on purpose: the GPU tests allow the
device a multiple of the twin's own distance from float64).

Also here: the over-smoothing experiment of DESIGN.md section 28 -- seeded AR(1) "natural" trajectories, a "generated"
version smoothed along time and shrunk towards its mean, a model fitted on 12 utterances and applied to 6 held-out ones."""
import numpy as np

L, H, M = 64, 32, 33
TINY = 2.0 ** -40
FLOOR = float(np.float32(1e-20))
F32_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24
ST_WAVES, MS_WAVES = 8, 4           # the device's interleaved partial sums (the Higham-style bounds of the GPU tests use them)


def window(dtype=np.float64):
    """w[t] = 0.5 - 0.5 cos(2 pi t / 64): made in float64, rounded to float32 once (the device's constants), then cast."""
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)).astype(np.float32)
    w[16] = w[48] = 0.5
    return w.astype(dtype)


def clamp_n(n_frames, B, maxF):
    if n_frames is None:
        return [maxF] * B
    return [int(min(max(int(v), 0), maxF)) for v in n_frames]


def _matrices(dtype):
    t, m = np.arange(L)[:, None], np.arange(M)[None, :]
    ang = 2.0 * np.pi * t * m / L
    wgt = np.where((m == 0) | (m == M - 1), 1.0, 2.0) / L
    return (np.cos(ang).T.astype(dtype), (-np.sin(ang)).T.astype(dtype),            # forward [33, 64]: Re, Im
            (wgt * np.cos(ang)).astype(dtype), (-wgt * np.sin(ang)).astype(dtype))  # inverse [64, 33]: from Re, from Im


def traj_stats(x, n_frames=None, dtype=np.float64):
    """x [B, maxF, C] -> [B, C, 2] (mean about the first frame, population variance about that mean)."""
    B, maxF, C = x.shape
    out = np.zeros((B, C, 2), dtype)
    for b, n in enumerate(clamp_n(n_frames, B, maxF)):
        if n == 0:
            continue
        xb = x[b, :n].astype(dtype)
        mean = xb[0] + (xb - xb[0]).sum(0, dtype=dtype) / dtype(n)
        d = xb - mean
        out[b, :, 0], out[b, :, 1] = mean, (d * d).sum(0, dtype=dtype) / dtype(n)
    return out


def gv_gain_minus_1(stats_b, gv_t, alpha, g_max, dtype):
    mean, var, gv_t = stats_b[:, 0].astype(dtype), stats_b[:, 1].astype(dtype), np.asarray(gv_t).astype(dtype)
    ok = (var > dtype(TINY)) & (gv_t > 0)
    with np.errstate(all='ignore'):
        q = np.where(ok, gv_t / np.where(ok, var, 1), 1).astype(dtype)
        ok &= q <= dtype(F32_MAX)
        g = dtype(1) + dtype(alpha) * (np.sqrt(np.where(ok, q, 1)).astype(dtype) - dtype(1))
    g = np.minimum(np.maximum(g, dtype(1) / dtype(g_max)), dtype(g_max))
    return np.where(ok, g - dtype(1), 0).astype(dtype)


def gv_filter(x, n_frames, stats, gv_t, alpha, g_max, dtype=np.float64):
    B, maxF, C = x.shape
    y = np.zeros(x.shape, dtype)
    for b, n in enumerate(clamp_n(n_frames, B, maxF)):
        xb = x[b, :n].astype(dtype)
        d = gv_gain_minus_1(stats[b], gv_t, alpha, g_max, dtype) * (xb - stats[b, :, 0].astype(dtype))
        y[b, :n] = np.where(d == 0, xb, xb + d)
    return y


def segment_index(n):
    """[J + 1, 64] frame indices of the segments j = 0 .. J = ceil(n / 32) of an utterance of n >= 1 frames (edge hold)."""
    J = (n + H - 1) // H
    return np.clip(H * np.arange(J + 1)[:, None] - H + np.arange(L)[None, :], 0, n - 1)


def spectra(xb, mean, dtype=np.float64):
    """xb [n, C], mean [C] -> (v [J + 1, 64, C], Re X, Im X [J + 1, 33, C])."""
    fr, fi, _, _ = _matrices(dtype)
    v = window(dtype)[None, :, None] * (xb.astype(dtype)[segment_index(len(xb))] - mean.astype(dtype))
    return v, np.matmul(fr[None], v), np.matmul(fi[None], v)


def _log_power(re, im, dtype):
    p = re * re + im * im
    ok = (p > dtype(FLOOR)) & (p <= dtype(F32_MAX))
    return ok, np.log(np.where(ok, p, 1)).astype(dtype)


def ms_stats(x, n_frames, stats, dtype=np.float64):
    """-> [B, C, 33, 3] (count, sum s, sum s^2)."""
    B, maxF, C = x.shape
    out = np.zeros((B, C, M, 3), dtype)
    for b, n in enumerate(clamp_n(n_frames, B, maxF)):
        if n == 0:
            continue
        _, re, im = spectra(x[b, :n], stats[b, :, 0], dtype)
        ok, s = _log_power(re, im, dtype)
        s = np.where(ok, s, dtype(0))
        out[b, :, :, 0] = ok.sum(0).T
        out[b, :, :, 1] = s.sum(0, dtype=dtype).T
        out[b, :, :, 2] = (s * s).sum(0, dtype=dtype).T
    return out


def ms_filter(x, n_frames, stats, coef, lo, hi, dtype=np.float64, counts=None):
    """coef [C, 33, 2].  counts: a dict that receives 'gains' (bins m >= 1 above the floor) and 'clamped' among them."""
    B, maxF, C = x.shape
    _, _, ir, ii = _matrices(dtype)
    a, bb = coef[:, :, 0].T.astype(dtype)[None], coef[:, :, 1].T.astype(dtype)[None]
    y = np.zeros(x.shape, dtype)
    n_gain = n_clamp = 0
    for b, n in enumerate(clamp_n(n_frames, B, maxF)):
        if n == 0:
            continue
        xb = x[b, :n].astype(dtype)
        _, re, im = spectra(xb, stats[b, :, 0], dtype)
        ok, s = _log_power(re, im, dtype)
        ok[:, 0] = False                                             # g_0 = 1
        e = np.where(ok, a * s + bb, 0).astype(dtype)
        ec = np.minimum(np.maximum(e, dtype(lo)), dtype(hi))
        n_gain, n_clamp = n_gain + int(ok.sum()), n_clamp + int((ok & (e != ec)).sum())
        g1 = np.where(ok, np.exp(ec).astype(dtype) - dtype(1), 0).astype(dtype)
        c = np.matmul(ir[None], g1 * re) + np.matmul(ii[None], g1 * im)            # [J + 1, 64, C]
        d = (c[:-1, H:] + c[1:, :H]).reshape(-1, C)[:n]                            # the earlier segment first
        y[b, :n] = np.where(d == 0, xb, xb + d)
    if counts is not None:
        counts['gains'], counts['clamped'] = n_gain, n_clamp
    return y


# ------------------------------------------------------------------------------------------ the over-smoothing experiment
def smooth_and_shrink(x, taps=(0.2, 0.6, 0.2), shrink=0.8):
    """What a decoder trained on a squared error does to a trajectory, in caricature: smoothed along time (edge hold), then
    pulled towards its mean."""
    p = np.concatenate([x[:1], x, x[-1:]], 0)
    s = taps[0] * p[:-2] + taps[1] * p[1:-1] + taps[2] * p[2:]
    m = s.mean(0)
    return m + shrink * (s - m)


def corpus(seed=28, n_utt=18, C=8, rho=0.9):
    """n_utt pairs (natural, generated) [n, C] float64, 300 <= n <= 900: AR(1) trajectories with pole rho around 0.45, the
    deviation growing with the channel from 0.05 to 0.12."""
    rng = np.random.default_rng(seed)
    sigma = np.linspace(0.05, 0.12, C)
    out = []
    for _ in range(n_utt):
        n = int(rng.integers(300, 901))
        e = rng.standard_normal((n + 64, C))
        z = np.zeros_like(e)
        for t in range(1, len(e)):
            z[t] = rho * z[t - 1] + np.sqrt(1.0 - rho * rho) * e[t]
        nat = 0.45 + sigma * z[64:]
        out.append((nat, smooth_and_shrink(nat)))
    return out


def _batch(items):
    n = [len(v) for v in items]
    x = np.zeros((len(items), max(n), items[0].shape[1]))
    for b, v in enumerate(items):
        x[b, :len(v)] = v
    return x, n


def mean_log_ms_db(x, n):
    """[C, 33]: the mean over all segments of 10 log10 |X|^2."""
    ms = ms_stats(x, n, traj_stats(x, n)).sum(0)
    return (10.0 / np.log(10.0)) * ms[:, :, 1] / np.maximum(ms[:, :, 0], 1)


def experiment(k=1.0, max_db=20.0, n_fit=12):
    """Fits on the first n_fit pairs, filters the held-out generated ones in float64; returns the five figures of DESIGN.md
    section 28 and what they are ratios of."""
    import postfilter
    pairs = corpus()
    (xn, nn), (xg, ng) = _batch([p[0] for p in pairs[:n_fit]]), _batch([p[1] for p in pairs[:n_fit]])
    sn, sg = traj_stats(xn, nn), traj_stats(xg, ng)
    model = postfilter.model_from_stats([(sn, nn)], [ms_stats(xn, nn, sn)], [ms_stats(xg, ng, sg)])
    coef = postfilter.ms_coef(model, k).astype(np.float64)
    (hn, hnn), (hg, hgn) = _batch([p[0] for p in pairs[n_fit:]]), _batch([p[1] for p in pairs[n_fit:]])
    hi = max_db * np.log(10.0) / 20.0
    counts = {}
    y = ms_filter(hg, hgn, traj_stats(hg, hgn), coef, -hi, hi, counts=counts)
    target = (10.0 / np.log(10.0)) * model.mu_N
    dist = lambda x, n: float(np.sqrt(((mean_log_ms_db(x, n) - target)[:, 1:] ** 2).mean()))
    valid = np.arange(hn.shape[1])[None, :, None] < np.array(hnn)[:, None, None]
    rms = lambda x: float(np.sqrt((((x - hn) ** 2) * valid).sum() / (valid.sum() * hn.shape[2])))
    var = lambda x, n: traj_stats(x, n)[:, :, 1]
    r = dict(d_gen=dist(hg, hgn), d_out=dist(y, hgn), d_nat=dist(hn, hnn), e_gen=rms(hg), e_out=rms(y),
             var_gen=float((var(hg, hgn) / var(hn, hnn)).mean()), var_out=float((var(y, hgn) / var(hn, hnn)).mean()),
             clamped=counts['clamped'] / max(counts['gains'], 1))
    r.update(ms_ratio_gen=r['d_out'] / r['d_gen'], ms_ratio_nat=r['d_out'] / r['d_nat'], err_ratio=r['e_out'] / r['e_gen'])
    return r
