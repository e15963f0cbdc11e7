"""numpy restatement of the harmonic-plus-noise vocoder (include/vc_hip.h, "Harmonic-plus-noise vocoder"): integers exact,
float64 for the envelope and the synthesis, and a float32 error model in the style of vocoder_kernels_ref / diff_ref: a sum of
n float32 terms carries (n + 8) u sum |t_i|, u = 2^-24.  Test infrastructure only."""
import numpy as np

import philox_ref

U = 2.0 ** -24
EXP2_ULPS = 2               # the device's exp2f, units in the last place (diff_ref.EXP2_ULPS)
LOG_ULPS = 2                # ... and its logf
MAX_HARMONICS = 256
SQRT12 = np.float32(np.sqrt(12.0))
# cos(2 pi x) on the device: z = 1/4 - |x - rint(x)|, z * P(z^2); the coefficients of csrc/vc_hnm.hip cos_turns
COS_COEF = np.array([6.2831854820251465, -41.34168243408203, 81.60247802734375, -76.58128356933594, 39.76072311401367],
                    np.float32)
COS_POLY_ERR = 4e-8         # |z P(z^2) - sin(2 pi z)| on [-1/4, 1/4] in exact arithmetic (test_hnm_cpu measures 3.1e-8)
# ... plus z's rounding (half an ulp of 1/4, times the slope 2 pi) and five fused steps and a product at a value <= 1
COS_ERR = COS_POLY_ERR + 2.0 * np.pi * 2.0 ** -26 + 8 * U


def window(win_length, n_fft):
    """The vocoder plan's padded periodic Hann window as the device holds it (float32 values, float64 array)."""
    i = np.arange(win_length)
    w = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    w[lp:lp + win_length] = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / win_length)).astype(np.float32)
    return w


def table(n_fft):
    """float32 [N, 2]: (cos, sin)(2 pi m / N), made in float64 -- the table vc_env_cepstral_f32 takes."""
    m = np.arange(n_fft)
    return np.stack([np.cos(2.0 * np.pi * m / n_fft), np.sin(2.0 * np.pi * m / n_fft)], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------ envelope
def _env_mats(N, L, tab):
    t = np.asarray(tab, np.float64)
    nb = N // 2 + 1
    k = np.arange(nb)
    n = np.arange(L + 1)
    idx = (n[:, None] * k[None, :]) % N
    w = np.full(nb, 2.0)
    w[0] = w[-1] = 1.0
    C = t[idx, 0] * w[None, :] / N                      # c = C @ A            [L + 1, nb]
    g = np.full(L + 1, 2.0)
    g[0] = 1.0
    Ec = t[idx, 0].T * g[None, :]                       # E = Ec @ c           [nb, L + 1]
    Th = -t[idx, 1].T * g[None, :]
    Th[:, 0] = 0.0
    return C, Ec, Th


def envelope(amp, n_fft, order, iters, floor, tab=None):
    """amp [F, nb] float32 -> (env_log, theta, bound_env, bound_theta, margin); float64 [F, nb] each, margin a number.
    The float32 model.  a carries LOG_ULPS ulp.  One pass is A -> c = C A -> E = Ec c: c_n is a sum of nb terms and the edge
    pair, (nb + 8) u sum |C_nk A_k|, E_k of L + 1 terms, (L + 9) u sum |Ec_kn c_n|, and c's own error reaches E through |Ec|:
    together the pass's LOCAL error.  An error d of A reaches E through S = Ec C, bounded two ways -- bin by bin through |S|,
    and in the norm |d|_w = sqrt(sum w_k d_k^2) (w = 1, 2, .., 2, 1), in which S is an orthogonal projection and does not
    enlarge it; |(S d)_k| <= sqrt(sum_j S_kj^2 / w_j) |d|_w -- and the smaller one is taken.  Through A = max(a, E) an error
    passes unchanged where E is taken, not at all where a is taken by more than the two bounds together, and is at most the
    larger of the two where they are nearer than that (max is 1-Lipschitz), so the bound holds whichever branch the device
    takes.  margin: the smallest |a - E| / (bound of a + bound of E) over all max steps (inf with iters == 0); above 1 the
    device provably took the reference's branch everywhere."""
    N, L = int(n_fft), int(order)
    tab = table(N) if tab is None else tab
    C, Ec, Th = _env_mats(N, L, tab)
    aC, aEc, aTh = np.abs(C), np.abs(Ec), np.abs(Th)
    nb = N // 2 + 1
    w = np.full(nb, 2.0)
    w[0] = w[-1] = 1.0
    S, Ts = Ec @ C, Th @ C
    aS, aTs = np.abs(S), np.abs(Ts)
    rS, rT = np.sqrt((S * S / w).sum(axis=1)), np.sqrt((Ts * Ts / w).sum(axis=1))
    wnorm = lambda v: np.sqrt((w * v * v).sum(axis=1))
    x = np.maximum(np.asarray(amp, np.float32), np.float32(floor)).astype(np.float64)
    a = np.log(x)
    ba = 2 * LOG_ULPS * U * np.abs(a) + 2 * U
    A, bA, rA = a, ba, wnorm(ba)
    margin = np.inf
    for p in range(int(iters) + 1):
        c = A @ C.T
        locc = (nb + 8) * U * (np.abs(A) @ aC.T)
        E = c @ Ec.T
        locE = locc @ aEc.T + (L + 9) * U * (np.abs(c) @ aEc.T)
        bE = np.minimum(bA @ aS.T, rA[:, None] * rS[None, :]) + locE
        if p == iters:
            bth = np.minimum(bA @ aTs.T, rA[:, None] * rT[None, :]) + locc @ aTh.T + (L + 9) * U * (np.abs(c) @ aTh.T)
            return E, c @ Th.T, bE, bth, margin
        gap = a - E
        tot = bE + ba
        margin = min(margin, float((np.abs(gap) / tot).min()))
        A = np.maximum(a, E)
        bA = np.where(gap > tot, ba, np.where(gap < -tot, bE, np.maximum(ba, bE)))
        rA = np.minimum(wnorm(bA), rA + wnorm(locE) + wnorm(ba))


# ------------------------------------------------------------------------------------------ plan
def plan(f0, n_frames, sr, hop, f0_lo=40.0, f0_hi=None):
    """f0 [F] float32 -> dict(voiced uint8, inc uint32, slope int32, phase uint32 [F], flags int): exact."""
    f0 = np.asarray(f0, np.float32)
    F = len(f0)
    nF = min(max(int(n_frames), 0), F)
    lo = np.float32(f0_lo)
    hi = np.float32(sr / 4.0 if f0_hi is None else f0_hi)
    kinc = np.float32(2.0 ** 32 / sr)
    x = f0[:nF]
    with np.errstate(invalid='ignore'):
        v = (x >= lo) & (x <= hi)
        flags = int(np.any(~v & (x != 0)))
        raw = np.rint(np.where(v, x, np.float32(0)) * kinc).astype(np.uint64)
    voiced = np.zeros(F, np.uint8)
    voiced[:nF] = v
    inc = np.zeros(F, np.uint64)
    idx = np.nonzero(v)[0]
    if len(idx):
        last = np.maximum.accumulate(np.where(v, np.arange(nF), -1))
        inc[:nF] = raw[np.where(last >= 0, last, idx[0])]
    slope = np.zeros(F, np.int64)
    if nF > 1:
        slope[:nF - 1] = np.floor_divide(inc[1:nF].astype(np.int64) - inc[:nF - 1].astype(np.int64), hop)
    step = (hop * inc.astype(np.int64) + slope * (hop * (hop - 1) // 2)) % (1 << 32)
    phase = np.zeros(F, np.int64)
    if nF > 1:
        phase[1:nF] = np.cumsum(step[:nF - 1]) % (1 << 32)
    return dict(voiced=voiced, inc=inc.astype(np.uint32), slope=slope.astype(np.int32), phase=phase.astype(np.uint32), flags=flags)


def sample_phase(pl, hop, f, j):
    """Phase (units of 2^-32 turn, Python ints / int64 arrays) at sample f * hop + j by the closed form."""
    j = np.asarray(j, np.int64)
    return (int(pl['phase'][f]) + j * int(pl['inc'][f]) + int(pl['slope'][f]) * (j * (j - 1) // 2)) % (1 << 32)


# ------------------------------------------------------------------------------------------ noise
def noise(seed, utt_id, n):
    """float32 [n]: what vc_noise_init_f32 writes for the first n samples of an utterance."""
    n = int(n)
    blocks = (n + 3) // 4
    words = philox_ref.philox4x32_10((np.arange(blocks), np.uint32(int(utt_id) & 0xFFFFFFFF), 0, 0),
                                     (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    x = np.stack(words, axis=1).reshape(-1)[:n]
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (SQRT12 * (u - np.float32(0.5))).astype(np.float32)


def noise_gain(env_log, voiced, n_frames, cutoff_bin, gscale):
    """(G float64 [F, nb], relative bound): gscale * exp(env_log) where noise goes, 0 elsewhere.  The exponent
    env_log * float32(log2 e) carries 2 u |env_log| log2(e) (the constant's rounding, the product's), times ln 2; exp2f
    EXP2_ULPS ulp; the product with gscale one rounding."""
    e = np.asarray(env_log, np.float32).astype(np.float64)
    F, nb = e.shape
    on = np.zeros((F, nb), bool)
    nF = min(max(int(n_frames), 0), F)
    on[:nF] = (np.asarray(voiced[:nF]) == 0)[:, None] | (np.arange(nb) >= cutoff_bin)[None, :]
    G = np.where(on, float(np.float32(gscale)) * np.exp(e), 0.0)
    return G, 2 * U * np.abs(e) + (2 * EXP2_ULPS + 1) * U


# ------------------------------------------------------------------------------------------ synthesis
def cos_turns_f64(x):
    """The device's polynomial evaluated in float64 (its approximation error alone)."""
    x = x - np.rint(x)
    z = 0.25 - np.abs(x)
    s = z * z
    p = np.zeros_like(s)
    for c in COS_COEF[::-1].astype(np.float64):
        p = p * s + c
    return z * p


def _lerp(row, pos_q, nb):
    """row float64 [nb] at the fixed-point positions pos_q (int64, units of 2^-32 bin): (value, |row| bracket for bounds)."""
    i0 = np.minimum(pos_q >> 32, nb - 1)
    i1 = np.minimum(i0 + 1, nb - 1)
    fr = (pos_q & 0xFFFFFFFF) * 2.0 ** -32
    return row[i0] + fr * (row[i1] - row[i0]), np.abs(row[i0]) + 2 * fr * (np.abs(row[i1]) + np.abs(row[i0]))


def synth(env_log, theta, pl, n_frames, n_fft, hop, cutoff_inc, scale, add=None):
    """(y float64 [hop (F - 1)], bound): the definition on the float32 inputs, and the float32 model of the device:
      amplitude   the interpolated exponent e carries 4 u on the bracket |e0| + 2 fr (|e0| + |e1|) (the fraction's conversion,
                  the difference, the fused step); times float32(log2 e) 2 u |e|; exp2f EXP2_ULPS ulp; the scale and the
                  interpolation between the ends 3 u: relative (6 |e| + 2 EXP2_ULPS + 4) u on either end
      angle       k phi converted to float32 at most 2^-26 turn; t (bracketed as e) 4 u; t / (2 pi) fused 3 u |t| / (2 pi)
      cosine      COS_ERR
      sum         (K + 8) u sum |a_k|, and one more rounding for add."""
    env_log = np.asarray(env_log, np.float32).astype(np.float64)
    theta = np.asarray(theta, np.float32).astype(np.float64)
    F, nb = env_log.shape
    N = int(n_fft)
    nF = min(max(int(n_frames), 0), F)
    L = hop * (F - 1)
    y = np.zeros(L)
    bound = np.zeros(L)
    sc = float(np.float32(scale))
    inc = pl['inc'].astype(np.int64)
    Ke = np.where((pl['voiced'] != 0) & (inc > 0), np.minimum((int(cutoff_inc) - 1) // np.maximum(inc, 1), MAX_HARMONICS), 0)
    j = np.arange(hop, dtype=np.int64)
    u = (j.astype(np.float32) / np.float32(hop)).astype(np.float64)
    for f in range(max(nF - 1, 0)):
        K0, K1 = int(Ke[f]), int(Ke[f + 1])
        K = max(K0, K1)
        phi = sample_phase(pl, hop, f, j)
        acc = np.zeros(hop)
        sa = np.zeros(hop)
        err = np.zeros(hop)
        for k in range(1, K + 1):
            ends = []
            for e, Kk in ((f, K0), (f + 1, K1)):
                if k <= Kk:
                    q = (k * int(inc[e])) * N
                    el, eb = _lerp(env_log[e], np.int64(q), nb)
                    tl, tb = _lerp(theta[e], np.int64(q), nb)
                    ends.append((sc * np.exp(el), (6 * eb + 2 * EXP2_ULPS + 4) * U, tl, 4 * U * tb))
                else:
                    ends.append(None)
            (a0, ra0, t0, bt0), (a1, ra1, t1, bt1) = [ends[i] if ends[i] is not None else (0.0, 0.0) + ends[1 - i][2:] for i in (0, 1)]
            a = a0 + u * (a1 - a0)
            t = t0 + u * (t1 - t0)
            ea = (np.abs(a0) * ra0 + np.abs(a1) * ra1) + 3 * U * (np.abs(a0) + np.abs(a1))
            et = bt0 + bt1 + 3 * U * (np.abs(t0) + np.abs(t1))
            turns = ((k * phi) % (1 << 32)) * 2.0 ** -32
            acc += a * np.cos(2.0 * np.pi * turns + t)
            sa += np.abs(a) + ea
            err += ea + (np.abs(a) + ea) * (COS_ERR + 2.0 * np.pi * (2.0 ** -26 + 3 * U * np.abs(t) / (2.0 * np.pi)) + et)
        lo = f * hop
        y[lo:lo + hop] = acc
        bound[lo:lo + hop] = err + (K + 8) * U * sa
        if add is not None:
            av = np.asarray(add[lo:lo + hop], np.float32).astype(np.float64)
            y[lo:lo + hop] = acc + av if K > 0 else av               # add itself, its negative zeros included
            bound[lo:lo + hop] += U * (np.abs(acc) + np.abs(av) + bound[lo:lo + hop]) if K > 0 else 0.0
    return y, bound


# ------------------------------------------------------------------------------------------ experiments
def stft_mag(x, w, hop):
    """|STFT| [1 + len // hop, nb] in librosa's sense (center=True, reflect padding), float64."""
    N = len(w)
    xp = np.pad(np.asarray(x, np.float64), N // 2, mode='reflect')
    F = 1 + len(x) // hop
    fr = np.stack([xp[f * hop:f * hop + N] for f in range(F)]) * w[None, :]
    return np.abs(np.fft.rfft(fr, axis=1))


def vowel(f0_hz, F, sr=16000, n_fft=400, vib=0.1, vib_hz=5.0, hop=80, phase0=0.0):
    """The round-trip case: (amp float32 [F, nb], f0 float32 [F], env float64 [nb]) -- a four-formant all-pole envelope and a
    contour with +-vib vibrato."""
    nb = n_fft // 2 + 1
    wk = np.pi * np.arange(nb) / (nb - 1)
    den = np.ones(nb, complex)
    for fc, bw in ((700.0, 300.0), (1220.0, 300.0), (2600.0, 400.0), (3500.0, 400.0)):
        r = np.exp(-np.pi * bw / sr)
        th = 2.0 * np.pi * fc / sr
        den *= (1 - 2 * r * np.cos(th) * np.exp(-1j * wk) + r * r * np.exp(-2j * wk))
    env = 0.05 / np.abs(den)
    t = np.arange(F) * hop / sr
    f0 = (f0_hz * (1.0 + vib * np.sin(2.0 * np.pi * vib_hz * t + phase0))).astype(np.float32)
    return np.tile(env.astype(np.float32), (F, 1)), f0, env


def db_rms(est_log, env, f0_hz, sr, n_fft, hi_hz=7400.0):
    """(rms, mean) in dB of est_log [F, nb] (natural log) against env [nb] over bins between 1.2 f0 and hi_hz."""
    k = np.arange(n_fft // 2 + 1) * sr / n_fft
    sel = (k >= 1.2 * f0_hz) & (k <= hi_hz)
    d = (20.0 / np.log(10.0)) * (est_log[:, sel] - np.log(env[sel])[None, :])
    return float(np.sqrt((d ** 2).mean())), float(d.mean())


EDGE = 3                    # frames left out at either end of a round trip: the STFT's reflect padding


def chain(amp, f0, sr=16000, n_fft=400, hop=80, order=24, iters=16, floor=1e-5, cutoff_hz=8000.0, f0_lo=40.0):
    """hnm_synth_batch(noise=False) for one utterance in float64: (y, env_log, theta, plan).  The envelope and the phase go
    through float32 on the way, as the device hands them from launch to launch."""
    F = len(f0)
    w = window(n_fft, n_fft)
    el, th = envelope(amp, n_fft, order, iters, floor)[:2]
    el, th = el.astype(np.float32), th.astype(np.float32)
    pl = plan(f0, F, sr, hop, f0_lo)
    cut = max(1, min(int(round(min(cutoff_hz, sr / 2.0) * 2.0 ** 32 / sr)), 2 ** 31))
    y = synth(el, th, pl, F, n_fft, hop, cut, np.float32(2.0 / w.sum()))[0]
    return y, el, th, pl


def round_trip_db(y, env, f0_hz, sr=16000, n_fft=400, hop=80, order=24, iters=16, floor=1e-5, estimate=None):
    """(rms, mean) dB of the envelope read back from the waveform y against env, interior frames.  estimate: the envelope
    estimator to use on the float32 STFT magnitudes [F, nb] (default: the reference's)."""
    S = stft_mag(y, window(n_fft, n_fft), hop).astype(np.float32)
    e = envelope(S, n_fft, order, iters, floor)[0] if estimate is None else estimate(S)
    return db_rms(np.asarray(e, np.float64)[EDGE:-EDGE], env, f0_hz, sr, n_fft)
