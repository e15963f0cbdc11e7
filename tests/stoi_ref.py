"""Numpy restatement of the intelligibility launches (include/vc_hip.h, "Intelligibility"): vc_stoi_energy_f32,
vc_stoi_keep_f32, vc_stoi_bands_f32, vc_stoi_score_f32 and vc_si_sdr_f32.  float64 by default.  With dtype=np.float32 the
band stage and the score stage are TWINS of the kernels: the same operations in the same order, each rounded once (numpy
never contracts a product into a sum), the transform the same radix-2 Stockham autosort.  Square roots and divisions
are correctly rounded on both sides, so a twin differs from the device by nothing or by an ulp here and there (the window
and the twiddles come from two float64 libraries); no test relies on bit equality with a twin.

The float64 band stage uses numpy's FFT on the MATERIALISED silence-removed signal, so it shares neither the fused gather
nor the transform with the kernel; ``frames_fused`` is the gather the kernel uses, tests/test_stoi_cpu.py pins the two to
1e-12.  ``band_bound`` is the float32 error model of T."""
import numpy as np

FS = 10000
W = 256
H = 128
NFFT = 512
N_SEG = 30
N_BANDS = 15
DYN = 40.0
EPS = 2.0 ** -52
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
U = 2.0 ** -24


def window(dtype=np.float64):
    """hanning(W + 2)[1 : -1] from float64, rounded once."""
    return np.hanning(W + 2)[1:-1].astype(dtype)


def n_frames(L):
    """Frames that start at i H for every i H < L - W."""
    L = int(L)
    return 0 if L <= W else -((W - L) // H)


def bands(fs=FS, n_fft=NFFT, n_bands=N_BANDS, f_min=150.0):
    """[n_bands, 2] (lo, hi): the half-open bin ranges of the one-third-octave bands (a loop, not evaluation.stoi_bands'
    broadcast)."""
    f = np.linspace(0.0, fs, n_fft + 1)[:n_fft // 2 + 1]
    out = np.zeros((n_bands, 2), np.int64)
    for j in range(n_bands):
        out[j, 0] = int(np.argmin(np.abs(f - f_min * 2.0 ** ((2 * j - 1) / 6.0))))
        out[j, 1] = int(np.argmin(np.abs(f - f_min * 2.0 ** ((2 * j + 1) / 6.0))))
    return out


def energies(x, L=None):
    """e[i] = sum((x[iH : iH + W] w)^2) over the frames of the first L samples, float64."""
    x = np.asarray(x, np.float64)
    L = len(x) if L is None else min(max(int(L), 0), len(x))
    w = window()
    return np.array([np.sum((x[i * H:i * H + W] * w) ** 2) for i in range(n_frames(L))], np.float64)


def kept(e, dyn=DYN):
    """The frames with e > max(e) 10^(-dyn / 10), ascending; none for no frame or digital silence."""
    e = np.asarray(e, np.float64)
    if e.size == 0:
        return np.zeros(0, np.int64)
    return np.nonzero(e > e.max() * 10.0 ** (-dyn / 10.0))[0].astype(np.int64)


def threshold_margin(e, dyn=DYN):
    """The smallest |e / threshold - 1| over the frames (inf for no frame or silence): the kept list is well conditioned
    when this is far above float32 rounding."""
    e = np.asarray(e, np.float64)
    if e.size == 0 or e.max() <= 0.0:
        return np.inf
    return float(np.min(np.abs(e / (e.max() * 10.0 ** (-dyn / 10.0)) - 1.0)))


def silence_removed(x, idx):
    """x_sil [(K + 1) H]: the overlap-add at hop H of the kept, windowed frames (float64)."""
    x = np.asarray(x, np.float64)
    w = window()
    out = np.zeros((len(idx) + 1) * H if len(idx) else 0)
    for k, i in enumerate(idx):
        out[k * H:k * H + W] += x[i * H:i * H + W] * w
    return out


def frames_materialised(x, idx):
    """[M, W], M = max(K - 1, 0): the frames of silence_removed(x), windowed again (float64)."""
    xs = silence_removed(x, idx)
    M = n_frames(len(xs))
    w = window()
    return np.array([xs[m * H:m * H + W] * w for m in range(M)], np.float64).reshape(M, W)


def frames_fused(x, idx, dtype=np.float64):
    """The same frames as the kernel gathers them from x through idx[m - 1], idx[m], idx[m + 1], in its operation order."""
    T = dtype
    x = np.asarray(x, T)
    w = window(T)
    M = max(len(idx) - 1, 0)
    z = np.zeros((M, W), T)
    for m in range(M):
        cur = w * x[idx[m] * H:idx[m] * H + W]
        lo = cur[:H] if m == 0 else w[H:] * x[idx[m - 1] * H + H:idx[m - 1] * H + W] + cur[:H]
        hi = cur[H:] + w[:H] * x[idx[m + 1] * H:idx[m + 1] * H + H]
        z[m] = np.concatenate([lo, hi]) * w
    return z


def twiddles(dtype=np.float32):
    t = np.arange(NFFT // 2, dtype=np.float64)
    return np.cos(2.0 * np.pi * t / NFFT).astype(dtype), (-np.sin(2.0 * np.pi * t / NFFT)).astype(dtype)


def stockham(z, dtype=np.float32):
    """The kernel's transform of z [M, W] (zero-padded to 512): (re, im) [M, 512] of ``dtype``."""
    T = dtype
    z = np.asarray(z, T)
    M = z.shape[0]
    wr, wi = twiddles(T)
    re, im = np.zeros((M, NFFT), T), np.zeros((M, NFFT), T)
    re[:, 0::2] = z
    re[:, 1::2] = z * wr
    im[:, 1::2] = z * wi
    j = np.arange(NFFT // 2)
    for st in range(1, 9):
        s = 1 << st
        q = j & (s - 1)
        ps = j - q
        ur, ui, vr_, vi = re[:, :256], im[:, :256], re[:, 256:], im[:, 256:]
        dr, di = ur - vr_, ui - vi
        nre, nim = np.zeros_like(re), np.zeros_like(im)
        nre[:, q + 2 * ps] = ur + vr_
        nim[:, q + 2 * ps] = ui + vi
        if st == 8:
            nre[:, q + 2 * ps + s], nim[:, q + 2 * ps + s] = dr, di
        else:
            nre[:, q + 2 * ps + s] = dr * wr[ps] - di * wi[ps]
            nim[:, q + 2 * ps + s] = dr * wi[ps] + di * wr[ps]
        re, im = nre, nim
    return re, im


def band_T(x, idx, tab=None, dtype=np.float64):
    """T [M, n_bands] of one signal through the list idx.  float64: numpy's FFT of the materialised frames.  float32: the
    kernel's twin (fused gather, Stockham transform, sums ascending in k)."""
    tab = bands() if tab is None else np.asarray(tab)
    if dtype == np.float64:
        fr = frames_materialised(x, idx)
        P = np.abs(np.fft.rfft(fr, NFFT, axis=1)) ** 2 if len(fr) else np.zeros((0, NFFT // 2 + 1))
        return np.sqrt(np.array([[P[m, lo:hi].sum() for lo, hi in tab] for m in range(len(fr))]).reshape(len(fr), len(tab)))
    T = dtype
    z = frames_fused(x, idx, T)
    re, im = stockham(z, T)
    P = re[:, :NFFT // 2 + 1] * re[:, :NFFT // 2 + 1] + im[:, :NFFT // 2 + 1] * im[:, :NFFT // 2 + 1]
    out = np.zeros((len(z), len(tab)), T)
    for j, (lo, hi) in enumerate(tab):
        acc = np.zeros(len(z), T)
        for k in range(lo, hi):
            acc = acc + P[:, k]
        out[:, j] = np.sqrt(acc)
    return out


def band_bound(x, idx, tab=None):
    """|T_device - T_float64| <= bound [M, n_bands], the float32 model of vc_stoi_bands_f32 (u = 2^-24).

    The frame: z = (w a + w b) w with w rounded once from float64 (relative u per factor, three factors per term), two
    products, one sum and one product each rounded once: |dz[n]| <= 7 u (|w a| + |w b|) w to first order.  The transform:
    nine radix-2 stages; a stage's butterfly is one complex sum and one complex product by a twiddle that is itself within u:
    Higham's bound for the FFT gives |dX|_2 <= 9 * g * |X|_2 over all 512 bins with g = (4 + sqrt 2) u per stage (sum u,
    product sqrt 2 u ... (1 + sqrt 2) u, twiddle u), and |X|_2 = sqrt(512) |z|_2; an input error dz reaches X as
    sqrt(512) |dz|_2.  A band's T is the 2-norm of a slice of X, so |dT| <= |dX|_2 whatever the slice.  Then the squares
    (2 products and a sum: 3 u relative on each |X[k]|^2), their sum over the band's n bins ((n - 1) u) and the root
    (halves the relative error, adds u): (n + 2) / 2 + 1 = (n + 4) / 2 u relative on T."""
    tab = bands() if tab is None else np.asarray(tab)
    x = np.asarray(x, np.float64)
    w = window()
    M = max(len(idx) - 1, 0)
    T = band_T(x, idx, tab)
    out = np.zeros((M, len(tab)))
    for m in range(M):
        cur = np.abs(w * x[idx[m] * H:idx[m] * H + W])
        lo = cur[:H] + (0.0 if m == 0 else np.abs(w[H:] * x[idx[m - 1] * H + H:idx[m - 1] * H + W]))
        hi = cur[H:] + np.abs(w[:H] * x[idx[m + 1] * H:idx[m + 1] * H + H])
        mag = np.concatenate([lo, hi]) * w
        dz = 7.0 * U * np.sqrt(np.sum(mag ** 2))
        dX = np.sqrt(NFFT) * (9.0 * (4.0 + np.sqrt(2.0)) * U * np.sqrt(np.sum(mag ** 2)) + dz)
        for j, (lo_k, hi_k) in enumerate(tab):
            out[m, j] = dX + 0.5 * (hi_k - lo_k + 4) * U * T[m, j]
    return out


def _norm(v, T, axis):
    """(v - mean) / (norm + eps) along ``axis``: sums ascending from +0 in dtype T."""
    n = v.shape[axis]
    v = np.moveaxis(v, axis, 0)
    acc = np.zeros(v.shape[1:], T)
    for i in range(n):
        acc = acc + v[i]
    c = v - acc / T(n)
    q = np.zeros(v.shape[1:], T)
    for i in range(n):
        q = q + c[i] * c[i]
    return np.moveaxis(c / (np.sqrt(q) + T(EPS)), 0, axis)


def segments(Tx, Ty, mode=0, dtype=np.float64):
    """seg [S], S = max(M - N + 1, 0), from T [M, n_bands] of both signals.  mode 0: STOI, 1: ESTOI."""
    T = dtype
    Tx, Ty = np.asarray(Tx, T), np.asarray(Ty, T)
    M, nb = Tx.shape
    S = max(M - N_SEG + 1, 0)
    seg = np.zeros(S, T)
    for s in range(S):
        x, y = Tx[s:s + N_SEG], Ty[s:s + N_SEG]                     # [N, nb]
        if mode == 0:
            sx, sy = np.zeros(nb, T), np.zeros(nb, T)
            for n in range(N_SEG):
                sx = sx + x[n] * x[n]
                sy = sy + y[n] * y[n]
            a = np.sqrt(sx) / (np.sqrt(sy) + T(EPS))
            yp = np.minimum(a[None, :] * y, T(CLIP) * x)
            prod = _norm(x, T, 0) * _norm(yp, T, 0)
            d = np.zeros(nb, T)
            for n in range(N_SEG):
                d = d + prod[n]
            acc = T(0.0)
            for j in range(nb):
                acc = acc + d[j]
            seg[s] = acc / T(nb)
        else:
            xr, yr = _norm(x, T, 0), _norm(y, T, 0)
            prod = _norm(xr, T, 1) * _norm(yr, T, 1)
            p = np.zeros(N_SEG, T)
            for j in range(nb):
                p = p + prod[:, j]
            acc = T(0.0)
            for n in range(N_SEG):
                acc = acc + p[n]
            seg[s] = acc / T(N_SEG)
    return seg


def score(seg):
    """The mean over the segments (float64 sum, as on the device), 0 for none; of the dtype of seg."""
    seg = np.asarray(seg)
    if seg.size == 0:
        return seg.dtype.type(0.0)
    return seg.dtype.type(np.sum(seg.astype(np.float64)) / seg.size)


def stoi(x, y, L=None, extended=False, dyn=DYN, tab=None, detail=False):
    """The chained float64 restatement: score, or (score, seg, idx, Tx, Ty) with detail."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    idx = kept(energies(x, L), dyn)
    Tx, Ty = band_T(x, idx, tab), band_T(y, idx, tab)
    seg = segments(Tx, Ty, 1 if extended else 0)
    return (score(seg), seg, idx, Tx, Ty) if detail else float(score(seg))


def stoi_twin(x, y, L=None, extended=False, dyn=DYN, tab=None):
    """The chained float32 twin on the float64 kept list: band twin, then score twin.  (score, seg) as float64 values."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    idx = kept(energies(x, L), dyn)
    seg = segments(band_T(x, idx, tab, np.float32), band_T(y, idx, tab, np.float32), 1 if extended else 0, np.float32)
    return float(score(seg)), seg.astype(np.float64)


def chain_distance(x, y, L=None, extended=False):
    """(score, seg, distance of seg, distance of score) between the float64 chain and its float32 twin: what a bound on
    stoi_batch end to end is a multiple of."""
    want, seg, _, _, _ = stoi(x, y, L, extended, detail=True)
    t_score, t_seg = stoi_twin(x, y, L, extended)
    return float(want), seg, float(np.abs(t_seg - seg).max()) if len(seg) else 0.0, abs(t_score - float(want))


def si_sdr(x, y, L=None, zero_mean=True):
    """(si_sdr in dB as float64, valid)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    L = len(x) if L is None else min(max(int(L), 0), len(x))
    x, y = x[:L], y[:L]
    if L and zero_mean:
        x, y = x - x.sum() / L, y - y.sum() / L
    sxx = float(np.sum(x * x))
    if L == 0 or sxx <= 0.0:
        return 0.0, 0
    a = float(np.sum(x * y)) / sxx
    num, r = a * a * sxx, float(np.sum((a * x - y) ** 2))
    if num == 0.0:
        return -np.inf, 1
    if r == 0.0:
        return np.inf, 1
    return 10.0 * np.log10(num / r), 1


def modulated_vowel(seconds=1.6, f0_hz=120.0, mod_hz=4.0, depth=0.8, sr=FS):
    """A three-formant /a/ (tests/diff_ref.py's resonator cascade) on a pulse train with vibrato, its amplitude modulated at
    a syllable rate: float64 [seconds * sr], peak 0.5."""
    import diff_ref
    n = int(seconds * sr)
    t = np.arange(n) / float(sr)
    f0 = f0_hz * (1.0 + 0.03 * np.sin(2.0 * np.pi * 5.0 * t))
    v = diff_ref.vowel(diff_ref.pulse_train(f0, sr, top=0.45 * sr), *diff_ref.VOWEL_A, sr=sr)
    v = v * (1.0 - depth * 0.5 * (1.0 + np.cos(2.0 * np.pi * mod_hz * t)))
    return 0.5 * v / np.abs(v).max()


def white_noise_at(x, snr_db, seed):
    """White noise at snr_db below the mean power of x."""
    x = np.asarray(x, np.float64)
    return np.sqrt(np.mean(x ** 2) / 10.0 ** (snr_db / 10.0)) * np.random.RandomState(seed).standard_normal(len(x))
