"""Host reference of dereverberation (include/vc_hip.h, "Dereverberation"): the WPE solver in float64
numpy IN THE HEADER'S ORDER of operations (the device is held to it bit for bit), the complex STFT and its inverse with the
project's framing (tests/diff_ref.py's, not a third copy), the float32 bounds of the two transform launches, a float32 twin
of the transforms, and the synthetic room corpus of the method's own check.  Plain numpy (scipy only for the vowels'
resonators and the convolution).  Nothing here is fitted to a device result.

Bounds the tests use, and where they come from
  stft      either component of a bin is a float32 sum whose longest chain is vr.chain_of(n_fft) additions:
            e = (chain + 8) u sum_n |w[n] x[n]|, u = 2^-24 -- the model of tests/vocoder_kernels_ref.py, as
            tests/denoise_ref.py power() uses it for vc_stft_power_f32 (stft_bound below is that e, nothing else).
  |Z|^2     the complex launch stores re and im; the power launch squares and adds the same two numbers in registers.  With
            identical re, im: a = fl(re re), b = fl(im im), uncontracted fl(a + b) is within u (a + b) of a + b; contracted
            fl(re re + b) differs from a + b by at most u |re re| from the unrounded first product, and is rounded once:
            within u (a + b) + u a.  So the two differ by at most 2 u (a + b) + u a <= 3 u P: 3 half-ulps, i.e. at most 2
            float32 ulps of the power (POWER_ULPS).  This presupposes that both launches hold the same re and im, i.e. that
            the compiler contracts the forward half alike in both: the complex kernel therefore repeats the power kernel's
            statements word for word (a first version that called a shared function did not, and was 4,906 ulps off on a
            small bin).  Measured on the device: 1 ulp at worst in every case.
  istft     the inverse half's own rounding on the spectrum it is given (vr.inverse_bound), through the overlap-add
            (vr.ola_of_bound), plus the overlap-add's own rounding (vr.ola_bound), trimmed: tests/diff_ref.py filter_bound
            without its forward and product terms (istft_bound below).
  wpe       none: bit for bit.
  end to end  the device's SI-SDR against the restatement's: twice the difference between the restatement and its float32
            twin on the same corpus, at least 0.05 dB (section 32's practice); the twin's figures are measured by
            tests/test_dereverb_cpu.py and written in profiles/dereverb/README.md.
"""
import functools

import numpy as np

import diff_ref
import vocoder_kernels_ref as vr

U = vr.U
POWER_ULPS = 2
MAX_TAPS, MAX_DELAY, MAX_ITERS, MAX_CONTEXT = 32, 64, 16, 8
LDS_BYTES = 160 * 1024


def max_frames(K):
    """vc_wpe_max_frames(K), restated."""
    return (LDS_BYTES - 8 * (2 * K * K + 2 * K + 4)) // 24 if 1 <= K <= MAX_TAPS else 0


def defaults(hop, sr, win, span_ms=80.0):
    """enhance.wpe_defaults, restated."""
    delay = -(-win // hop)
    taps = int(round(span_ms * sr / 1000.0 / hop))
    return min(max(taps, 1), MAX_TAPS), min(max(delay, 1), MAX_DELAY)


# ------------------------------------------------------------------------------------------ the solver
def _wpe_utt(xr32, xi32, F, K, D, I, c, floor_rel, load_rel, trace=None):
    """One utterance, all bins at once (they share F): xr32, xi32 [nb, >= F] float32 -> (yr, yi float32 [nb, F], taps float32
    [nb, K, 2], status int32 [nb]).  Vectorised over bins and over matrix entries; every sum walks its own index in a
    Python loop, so its order is the header's."""
    nb = xr32.shape[0]
    status = np.zeros(nb, np.int32)
    taps = np.zeros((nb, K, 2), np.float32)
    if F <= D:
        status[:] = 2
        return xr32[:, :F].copy(), xi32[:, :F].copy(), taps, status
    xr, xi = xr32[:, :F].astype(np.float64), xi32[:, :F].astype(np.float64)
    p = xr * xr + xi * xi
    m = np.zeros(nb)
    for t in range(F):
        m = m + p[:, t]
    lam0 = np.float64(np.float32(floor_rel)) * (m / np.float64(F))
    bad = np.zeros(nb, bool)
    yr = yi = None
    tt = np.arange(F)
    for _ in range(I):
        s, cnt = np.zeros((nb, F)), np.zeros(F)
        for off in range(-c, c + 1):
            ok = (tt + off >= 0) & (tt + off < F)
            s[:, ok] = s[:, ok] + p[:, tt[ok] + off]
            cnt[ok] += 1.0
        s = s / cnt
        lam = np.where(s > lam0[:, None], s, lam0[:, None])
        Rr, Ri = np.zeros((nb, K, K)), np.zeros((nb, K, K))
        qr, qi = np.zeros((nb, K)), np.zeros((nb, K))
        for t in range(D, F):
            n = min(K, t - D + 1)
            idx = t - D - np.arange(n)
            ar, ai = xr[:, idx], xi[:, idx]                                  # xt_t[i], i < n
            l = lam[:, t]
            pr = ar[:, :, None] * ar[:, None, :] + ai[:, :, None] * ai[:, None, :]
            pi = ai[:, :, None] * ar[:, None, :] - ar[:, :, None] * ai[:, None, :]
            Rr[:, :n, :n] = Rr[:, :n, :n] + pr / l[:, None, None]
            Ri[:, :n, :n] = Ri[:, :n, :n] + pi / l[:, None, None]
            br, bi = xr[:, t, None], xi[:, t, None]
            qr[:, :n] = qr[:, :n] + (ar * br + ai * bi) / l[:, None]
            qi[:, :n] = qi[:, :n] + (ai * br - ar * bi) / l[:, None]
        tr = np.zeros(nb)
        for i in range(K):
            tr = tr + Rr[:, i, i]
        add = (np.float64(np.float32(load_rel)) * tr) / np.float64(K)
        for i in range(K):
            Rr[:, i, i] = Rr[:, i, i] + add
        if trace is not None:
            full = Rr + 1j * Ri
            iu = np.triu_indices(K, 1)
            full[:, iu[1], iu[0]] = np.conj(full[:, iu[0], iu[1]])
            trace.append((full, qr + 1j * qi))
        # R = L L^H by columns; only the upper triangle of R is read
        Lr, Li = np.zeros((nb, K, K)), np.zeros((nb, K, K))
        for j in range(K):
            d = Rr[:, j, j].copy()
            for k in range(j):
                d = d - (Lr[:, j, k] * Lr[:, j, k] + Li[:, j, k] * Li[:, j, k])
            bad |= ~((d > 0.0) & (d < np.inf))
            dj = np.sqrt(d)
            Lr[:, j, j] = dj
            if j + 1 < K:
                sr, si = Rr[:, j, j + 1:].copy(), -Ri[:, j, j + 1:]
                for k in range(j):
                    ar, ai = Lr[:, j + 1:, k], Li[:, j + 1:, k]
                    br, bi = Lr[:, j, k, None], Li[:, j, k, None]
                    sr = sr - (ar * br + ai * bi)
                    si = si - (ai * br - ar * bi)
                Lr[:, j + 1:, j] = sr / dj[:, None]
                Li[:, j + 1:, j] = si / dj[:, None]
        zr, zi = qr.copy(), qi.copy()
        for k in range(K):
            d = Lr[:, k, k]
            zr[:, k], zi[:, k] = zr[:, k] / d, zi[:, k] / d
            ar, ai = Lr[:, k + 1:, k], Li[:, k + 1:, k]
            br, bi = zr[:, k, None], zi[:, k, None]
            zr[:, k + 1:] = zr[:, k + 1:] - (ar * br - ai * bi)
            zi[:, k + 1:] = zi[:, k + 1:] - (ar * bi + ai * br)
        for k in range(K - 1, -1, -1):
            d = Lr[:, k, k]
            zr[:, k], zi[:, k] = zr[:, k] / d, zi[:, k] / d
            ar, ai = Lr[:, k, :k], Li[:, k, :k]                              # L[k][i], i < k
            br, bi = zr[:, k, None], zi[:, k, None]
            zr[:, :k] = zr[:, :k] - (ar * br + ai * bi)
            zi[:, :k] = zi[:, :k] - (ar * bi - ai * br)
        sr, si = np.zeros((nb, F)), np.zeros((nb, F))
        for i in range(K):
            ok = tt >= D + i
            ur, ui = xr[:, tt[ok] - D - i], xi[:, tt[ok] - D - i]
            gr, gi = zr[:, i, None], zi[:, i, None]
            sr[:, ok] = sr[:, ok] + (gr * ur + gi * ui)
            si[:, ok] = si[:, ok] + (gr * ui - gi * ur)
        yr, yi = xr - sr, xi - si
        p = yr * yr + yi * yi
    good = ~bad
    out_r, out_i = xr32[:, :F].copy(), xi32[:, :F].copy()
    out_r[good], out_i[good] = yr[good].astype(np.float32), yi[good].astype(np.float32)
    taps[good, :, 0], taps[good, :, 1] = zr[good].astype(np.float32), zi[good].astype(np.float32)
    status[bad] = 1
    return out_r, out_i, taps, status


def wpe_ref(re, im, n_frames=None, taps=16, delay=5, iterations=3, context=1, floor_rel=1e-6, load_rel=1e-8, trace=None):
    """vc_wpe_f32 restated: re, im [B, nb, maxF] float32; n_frames [B] or None (clamped to [0, maxF]).  Returns (out_re, out_im
    float32 [B, nb, maxF], taps float32 [B, nb, K, 2], status int32 [B, nb]).  trace: a list that receives per utterance and
    iteration the loaded normal equations (R [nb, K, K] complex128, q [nb, K])."""
    re, im = np.ascontiguousarray(re, np.float32), np.ascontiguousarray(im, np.float32)
    B, nb, maxF = re.shape
    out_r, out_i = np.zeros_like(re), np.zeros_like(im)
    tp, st = np.zeros((B, nb, taps, 2), np.float32), np.zeros((B, nb), np.int32)
    with np.errstate(all='ignore'):
        for b in range(B):
            F = maxF if n_frames is None else min(max(int(n_frames[b]), 0), maxF)
            r, i, tp[b], st[b] = _wpe_utt(re[b], im[b], F, taps, delay, iterations, context, floor_rel, load_rel, trace)
            out_r[b, :, :F], out_i[b, :, :F] = r, i
    return out_r, out_i, tp, st


# ------------------------------------------------------------------------------------------ the transforms
def stft(x, w, hop, n_use=None):
    """tests/diff_ref.py's stft, BIN-MAJOR: [bins, F] complex128."""
    return diff_ref.stft(x, w, hop, n_use).T


def istft(Z, w, hop):
    """tests/diff_ref.py's istft of a bin-major spectrum [bins, F]; the imaginary parts of bin 0 and bin N / 2 are ignored
    (numpy's irfft ignores them too; they are cleared here so that nobody has to know)."""
    S = np.array(Z, np.complex128).T
    S[:, 0], S[:, -1] = S[:, 0].real, S[:, -1].real
    return diff_ref.istft(S, w, hop)


def stft_bound(x, w, hop, F):
    """[F]: the bound on either component of every bin of frame f (see the top of this file)."""
    N = len(w)
    fr = vr._framed(np.asarray(x, np.float64), N, hop)[:F]
    return (vr.chain_of(N) + 8) * U * (np.abs(fr) * np.abs(w)).sum(axis=1)


def istft_bound(Z, w, hop):
    """(y float64 [hop (F - 1)], bound) of the device's float32 inverse on the float32 spectrum Z [bins, F] it is given."""
    N = len(w)
    S = np.array(Z, np.complex128).T
    S[:, 0], S[:, -1] = S[:, 0].real, S[:, -1].real
    fr = diff_ref.synthesis_frames(S, w)
    bound = vr.trim(vr.ola_of_bound(vr.inverse_bound(S, w), w, hop) + vr.ola_bound(fr, w, hop), N)
    return diff_ref.istft_frames(fr, w, hop), bound


def _dft_f32(N):
    k = np.arange(1 + N // 2)[:, None] * np.arange(N)[None, :]
    ang = 2.0 * np.pi * (k % N) / N
    return np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32)


def stft_f32(x, w, hop):
    """The float32 twin of stft: the same frames, window and transform with every product and sum in float32 (a direct
    transform by float32 matrix products).  (re, im) float32 [bins, F]."""
    N = len(w)
    fr = (vr._framed(np.asarray(x, np.float32), N, hop) * np.asarray(w, np.float32)).astype(np.float32)
    C, S = _dft_f32(N)
    return (C @ fr.T).astype(np.float32), (S @ fr.T).astype(np.float32)


def istft_f32(re, im, w, hop):
    """The float32 twin of istft: inverse transform, window, overlap-add and division in float32."""
    N = len(w)
    w32 = np.asarray(w, np.float32)
    C, S = _dft_f32(N)
    wt = np.full(1 + N // 2, 2.0, np.float32)
    wt[0] = wt[-1] = 1.0
    im = np.array(im, np.float32)
    im[0] = im[-1] = 0.0
    fr = ((C.T @ (wt[:, None] * np.asarray(re, np.float32)) + S.T @ (wt[:, None] * im)) / np.float32(N)).T * w32     # [F, N]
    F = fr.shape[0]
    y, wss = np.zeros(N + hop * (F - 1), np.float32), np.zeros(N + hop * (F - 1), np.float32)
    for f in range(F):
        y[f * hop:f * hop + N] += fr[f].astype(np.float32)
        wss[f * hop:f * hop + N] += w32 * w32
    ok = wss > vr.F32_TINY
    y[ok] /= wss[ok]
    return y[N // 2:N // 2 + hop * (F - 1)]


def dereverb(x, w, hop, twin=False, trace=None, **cfg):
    """The restatement end to end on one waveform x (float32 samples): stft -> float32 spectrum -> wpe_ref -> istft, the
    transforms in float64 (twin: in float32).  (y [hop (F - 1)], status [bins], taps)."""
    x = np.asarray(x, np.float32)
    if twin:
        re, im = stft_f32(x, w, hop)
    else:
        Z = stft(x.astype(np.float64), w, hop)
        re, im = Z.real.astype(np.float32), Z.imag.astype(np.float32)
    o_r, o_i, tp, st = wpe_ref(re[None], im[None], None, trace=trace, **cfg)
    if twin:
        return istft_f32(o_r[0], o_i[0], w, hop), st[0], tp[0]
    return istft(o_r[0].astype(np.float64) + 1j * o_i[0].astype(np.float64), w, hop), st[0], tp[0]


# ------------------------------------------------------------------------------------------ the room corpus
SR = 16000
EARLY_MS = 25.0


def dry_speech(seconds=2.5, sr=SR, seed=11):
    """Synthetic syllables, fully specified: /a/ /i/ /a/ ... of 0.2 s each while they fit, separated by 0.14 s pauses.  The
    excitation is a pulse train whose fundamental glides (110 -> 150 Hz, 140 -> 100 Hz, alternating) under a 3 % vibrato
    at 5 Hz, plus white noise at the pulse train's own RMS (a breathy voice); each syllable under a 20 ms raised-cosine onset
    and offset; in front of every second syllable a 30 ms burst of white noise at a quarter of the vowels' peak.
    float64 [seconds * sr], peak 0.5.

    The noise in the excitation is not decoration.  A pure pulse train through fixed resonators is a sum of slowly gliding
    sinusoids, predictable from its own past far beyond the 25 ms delay, and WPE then cancels the vowel itself: on the same
    corpus without it the restatement LOSES 1 dB after three iterations (measured while this file was written)."""
    rng = np.random.RandomState(seed)
    n = int(seconds * sr)
    x = np.zeros(n)
    seg, gap, ramp = int(0.2 * sr), int(0.14 * sr), int(0.02 * sr)
    env = np.ones(seg)
    env[:ramp] = 0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)
    env[-ramp:] = env[:ramp][::-1]
    pos, s = 0, 0
    while pos + seg <= n:
        t = np.arange(seg) / float(sr)
        lo, hi = (110.0, 150.0) if s % 2 == 0 else (140.0, 100.0)
        f0 = lo * (hi / lo) ** (np.arange(seg) / float(seg - 1)) * (1.0 + 0.03 * np.sin(2.0 * np.pi * 5.0 * t))
        e = diff_ref.pulse_train(f0, sr)
        e = e + np.sqrt((e * e).mean()) * rng.standard_normal(seg)
        fm = diff_ref.VOWEL_A if s % 2 == 0 else diff_ref.VOWEL_I
        x[pos:pos + seg] += env * diff_ref.vowel(e, *fm, sr=sr)
        if s % 2 == 1:
            nb = int(0.03 * sr)
            x[pos - nb:pos] += 0.125 * rng.standard_normal(nb) * np.hanning(nb)
        pos, s = pos + seg + gap, s + 1
    return 0.5 * x / np.abs(x).max()


def room(t60, drr_db=6.0, sr=SR, seed=23):
    """A unit direct path at sample 0 plus Gaussian noise from sample 1 on, its amplitude decaying by 60 dB in t60 seconds,
    cut at 1.2 t60 and scaled so that 1 / (energy of the tail) is drr_db.  float64."""
    n = int(1.2 * t60 * sr)
    h = np.random.RandomState(seed).standard_normal(n) * 10.0 ** (-3.0 * np.arange(n) / (t60 * sr))
    h[0] = 0.0
    h *= np.sqrt(10.0 ** (-drr_db / 10.0) / (h * h).sum())
    h[0] = 1.0
    return h


def corpus(t60, seconds=2.5, drr_db=6.0, sr=SR):
    """(reverberant, early) float32 [seconds * sr]: the dry speech through the room, and through its first 25 ms alone --
    the reference a dereverberator is scored against (direct sound and early reflections are kept on purpose).  Both scaled
    by one factor to a reverberant peak of 0.5."""
    from scipy import signal
    dry, h = dry_speech(seconds, sr), room(t60, drr_db, sr)
    n = len(dry)
    rev = signal.fftconvolve(dry, h)[:n]
    early = signal.fftconvolve(dry, h[:int(EARLY_MS * 1e-3 * sr)])[:n]
    g = 0.5 / np.abs(rev).max()
    return (g * rev).astype(np.float32), (g * early).astype(np.float32)


def condition_numbers(trace):
    """2-norm condition numbers of the loaded matrices in a wpe_ref trace, flat."""
    return np.concatenate([np.linalg.cond(R) for R, _ in trace])


T60S = (0.3, 0.6)
MIN_GAIN_DB = 2.0          # the least improvement of SI-SDR against the early reference, either room
E2E_FLOOR_DB = 0.05        # the least margin between the device's SI-SDR and the restatement's


def si_sdr(ref_wav, deg):
    import stoi_ref
    return stoi_ref.si_sdr(ref_wav, deg)[0]


@functools.lru_cache(maxsize=None)
def corpus_figures(t60):
    """The restatement and its float32 twin on one room of the corpus, computed once for every test that needs them: a dict
    with the waveforms (rev, early float32; n = the samples istft returns), the shipped configuration, y and y_twin, the
    status of every bin, the three SI-SDR figures against the early reference and the condition numbers of every loaded
    matrix the restatement factorised."""
    w = vr.device_window(vr.padded_window(400, 400))
    hop = 80
    K, D = defaults(hop, SR, 400)
    cfg = dict(taps=K, delay=D, iterations=3, context=1, floor_rel=1e-6, load_rel=1e-8)
    rev, early = corpus(t60)
    n = hop * (len(rev) // hop)
    trace = []
    y, status, _ = dereverb(rev, w, hop, trace=trace, **cfg)
    y32, status32, _ = dereverb(rev, w, hop, twin=True, **cfg)
    return dict(rev=rev, early=early, n=n, cfg=cfg, y=y, y_twin=y32, status=status, status_twin=status32,
                si_in=si_sdr(early[:n], rev[:n]), si_out=si_sdr(early[:n], y), si_twin=si_sdr(early[:n], y32),
                cond=condition_numbers(trace))
