"""Float64 reference of the Griffin-Lim vocoder kernels (csrc/vc_vocoder.hip), one launch at a time, on the kernels' own
state: the windowed synthesis frames  y_f[n] = w[n] * irfft(S_f)[n]  ([F, n_fft]) that an iteration launch reads and writes,
and the spectrum R [F, bins] it analyses them to.  Plain numpy; nothing of the project or of oracle/ is imported, so
tests/test_vocoder_kernels_cpu.py can hold this file against oracle/vocoder_oracle.py and tests/fgla_ref.py.

Arrays are frame-major like the C ABI ([F, bins], [F, n_fft]), the transpose of what librosa and the oracle work on.

The float32 model behind every bound here.  u = 2^-24.  An output that is a float32 sum of n terms t_i may be off by
(n + 8) u sum |t_i|; the 8 covers twiddle products, the window, the scale, rsqrtf and sincosf; n is the longest chain of
additions into one output:
    generic kernel, both halves   n_fft    one fmaf per sample (forward), two per bin 1 .. n_fft/2 - 1 plus the edge (inverse)
    400-point kernel, both halves 25 + 16  a 25-point and a 16-point stage, in either order
    overlap-add                   nov      = ceil(n_fft / hop) frames can cover one sample
    inverse pre-emphasis          1 / (1 - |coeff|), the geometric sum of the weights of the rounding errors fed back
    block sums                    the per-thread stride count plus the 16 per-wave partials
Where the input of a linear stage carries a bound of its own, that bound goes through the same linear map (with the absolute
values of its coefficients).  Nothing here is fitted to a device result.
"""
import functools

import numpy as np

U = 2.0 ** -24
F32_TINY = float(np.finfo(np.float32).tiny)
VG, VGG = 16, 4                  # frames per workgroup: 400-point kernel, generic kernel
PT = 1024                        # threads of the one-block-per-utterance kernels


# ------------------------------------------------------------------------------------------ sizes restated
def num_bins(n_fft):
    return 1 + n_fft // 2


def nov_of(n_fft, hop):
    return -(-n_fft // hop)


def tile_frames(n_fft):
    return VG if n_fft == 400 else VGG


def min_frames(n_fft, hop):
    """The smallest F with hop * (F - 1) > n_fft / 2 (the reflect padding fits)."""
    return (n_fft // 2) // hop + 2


def align256(x):
    return (x + 255) & ~255


def state_slots(n_fft):
    return 13 * 16 if n_fft == 400 else num_bins(n_fft)


def ws_layout(n_fft, hop, batch, max_frames, trace, momentum):
    """include/vc_hip.h next to vc_vocoder_workspace_bytes: (offset of frame buffer 1, offset of the two waveforms, their
    size each, offset of the state, total bytes)."""
    fb = align256(batch * max_frames * n_fft * 4)
    wb = align256(batch * hop * (max_frames - 1) * 4) if trace else 0
    o_state = 2 * fb + 2 * wb
    sb = align256(batch * max_frames * state_slots(n_fft) * 8) if momentum else 0
    return fb, 2 * fb, wb, o_state, o_state + sb + 256


def lds_bytes(n_fft, hop):
    """Dynamic LDS of an iteration launch: (400-point iteration, 400-point initial) or the generic kernel's one figure."""
    if n_fft == 400:
        base = 400 + 416 + 2 * (VG * 13) * 17
        return 4 * (base + (VG - 1) * hop + 400), 4 * (base + 2 * VG * 201)
    return 4 * (3 * n_fft + 2 * VGG * num_bins(n_fft) + (VGG - 1) * hop + n_fft)


# ------------------------------------------------------------------------------------------ window, frames, overlap-add
def padded_window(win_length, n_fft, taps=None):
    """float64 [n_fft]: the taps (periodic Hann when None) centred, lpad = (n_fft - win_length) // 2 zeros before them."""
    if taps is None:
        taps = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    taps = np.asarray(taps, np.float64)
    assert taps.shape == (win_length,) and win_length <= n_fft
    w = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    w[lpad:lpad + win_length] = taps
    return w


def device_window(w):
    """The table the plan uploads: the padded window rounded to float32 (widened again)."""
    return np.asarray(w, np.float32).astype(np.float64)


def frames_from_spectrum(S, w):
    """S [F, bins] complex -> w[n] * irfft(S_f)[n]  [F, n_fft]; the imaginary parts of the DC and Nyquist bins are ignored."""
    S = np.array(S, np.complex128)
    S[:, 0] = S[:, 0].real
    S[:, -1] = S[:, -1].real
    return np.fft.irfft(S, n=len(w), axis=1) * w


def overlap_add(frames, w, hop):
    """Untrimmed normalised overlap-add [n_fft + hop (F - 1)]: sum of the frames at f * hop, divided by the window's
    sum-square where that exceeds float32 tiny (librosa.istft), left as it is elsewhere."""
    F, N = frames.shape
    y = np.zeros(N + hop * (F - 1))
    wss = np.zeros_like(y)
    for f in range(F):
        y[f * hop:f * hop + N] += frames[f]
        wss[f * hop:f * hop + N] += w * w
    nz = wss > F32_TINY
    y[nz] /= wss[nz]
    return y


def trim(y, n_fft):
    """The n_fft / 2 samples the centred transform added at either end removed: hop (F - 1) samples."""
    return y[n_fft // 2:len(y) - n_fft // 2]


def waveform(frames, w, hop):
    return trim(overlap_add(frames, w, hop), frames.shape[1])


def _framed(wav, n_fft, hop):
    """[F, n_fft] view of the reflect-padded waveform, F = 1 + len(wav) // hop."""
    assert len(wav) > n_fft // 2, 'shorter than the reflect padding'
    yp = np.pad(wav, n_fft // 2, mode='reflect')
    F = 1 + (len(yp) - n_fft) // hop
    return yp[np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]]


def stft_wave(wav, w, hop):
    """librosa.stft(center=True, reflect) of a waveform, float64 throughout: [F, bins]."""
    return np.fft.rfft(_framed(np.asarray(wav, np.float64), len(w), hop) * w, axis=1)


def analysis(frames, w, hop):
    """R [F, bins]: the transform of the reflect-padded, trimmed overlap-add of a frame state."""
    return stft_wave(waveform(frames, w, hop), w, hop)


# ------------------------------------------------------------------------------------------ projection, one step
def unit(C):
    """C / |C|; a zero bin gets phase 0."""
    C = np.asarray(C, np.complex128)
    mag = np.abs(C)
    return np.where(mag > 0, C / np.where(mag > 0, mag, 1.0), 1.0 + 0.0j)


def project(C, amp):
    return amp * unit(C)


def step(frames_in, amp, w, hop, R_prev=None, beta=0.0):
    """One iteration launch: (R, frames_out) with R = analysis(frames_in), C = R - beta R_prev (R itself without R_prev),
    frames_out = frames(amp * unit(C))."""
    R = analysis(frames_in, w, hop)
    C = R if R_prev is None else R - beta * R_prev
    return R, frames_from_spectrum(project(C, amp), w)


def beta_of(momentum):
    """The float32 value the launcher computes: (float)(m / (1.0 + m)) with m the float32 momentum widened."""
    m = float(np.float32(momentum))
    return float(np.float32(m / (1.0 + m)))


def griffin_lim(amp, phase0, w, hop, num_iters, momentum=0.0, keep=None):
    """The whole loop on the frame state: returns the final frames.  keep: optional list that receives the frames after
    every launch."""
    frames = frames_from_spectrum(amp * np.exp(1j * np.asarray(phase0, np.float64)), w)
    beta, R_prev = beta_of(momentum), None
    if keep is not None:
        keep.append(frames)
    for i in range(1, num_iters):
        R, frames = step(frames, amp, w, hop, R_prev if momentum > 0 else None, beta)
        R_prev = R
        if keep is not None:
            keep.append(frames)
    return frames


# ------------------------------------------------------------------------------------------ the 400-point slot map
def slot_bins400():
    """[13, 16] int: slot (k1, k2) of the 400-point state holds bin k1 + 25 k2 of the 400-point spectrum."""
    return np.arange(13)[:, None] + 25 * np.arange(16)[None, :]


def slots_from_R400(R):
    """R [F, 201] -> [F, 13, 16]: the hermitian extension read in slot order (bins above 200 are conjugates)."""
    k = slot_bins400()
    full = np.concatenate([R, np.conj(R[:, -2:0:-1])], axis=1)               # [F, 400]
    return full[:, k]


def slot_amp400(amp):
    """amp [F, 201] -> [F, 13, 16]: the target magnitude of every slot."""
    k = slot_bins400()
    return np.asarray(amp)[:, np.where(k > 200, 400 - k, k)]


def spectrum_from_slots400(S):
    """S [F, 13, 16] complex, the projected slots -> the 400-point spectrum [F, 400] the kernel's inverse half transforms:
    the rows k1 = 13 .. 24 are the conjugates of rows 25 - k1 (bin 400 - k), the row k1 = 0 is taken as stored."""
    S = np.asarray(S, np.complex128)
    k = slot_bins400()
    X = np.zeros((S.shape[0], 400), np.complex128)
    X[:, k] = S
    X[:, 400 - k[1:]] = np.conj(S[:, 1:])
    return X


def frames_from_slots400(S, w):
    """The frames of the projected slots: the real part of the inverse transform of spectrum_from_slots400, windowed."""
    return np.fft.ifft(spectrum_from_slots400(S), axis=1).real * w


# ------------------------------------------------------------------------------------------ bounds
def chain_of(n_fft):
    """The longest chain of additions into one output of either half of the iteration kernel."""
    return 25 + 16 if n_fft == 400 else n_fft


def ola_abs(frames, w, hop):
    """The overlap-add of |frames| (untrimmed): sum |t_i| of the overlap-add, divided like the sum itself."""
    return overlap_add(np.abs(frames), w, hop)


def ola_bound(frames, w, hop):
    """Untrimmed [n_fft + hop (F - 1)]: the overlap-add's own rounding on given frames: (nov + 8) u sum |t_i| / wss."""
    return (nov_of(frames.shape[1], hop) + 8) * U * ola_abs(frames, w, hop)


def ola_of_bound(bound_frames, w, hop):
    """A per-sample bound on the frames pushed through the overlap-add (a linear map with non-negative coefficients)."""
    return overlap_add(bound_frames, w, hop)


def forward_bound(frames_in, w, hop):
    """[F]: bound on either component of every bin of R against analysis(frames_in).  With A[f] = sum_n w[n] a[f hop + n],
    a the reflect-padded trimmed overlap-add of |frames_in| (it dominates |x| sample by sample), the transform's own
    rounding is (chain + 8) u A and the overlap-add's, pushed through the transform, (nov + 8) u A."""
    N = frames_in.shape[1]
    a = trim(ola_abs(frames_in, w, hop), N)
    A = (_framed(a, N, hop) * np.abs(w)).sum(axis=1)
    return (chain_of(N) + 8 + nov_of(N, hop) + 8) * U * A


@functools.lru_cache(maxsize=1)
def _abs_twiddles(N):
    """(|cos(2 pi k n / N)|, |sin(2 pi k n / N)|), each [N/2 - 1, N], for the bins 0 < k < N/2."""
    ang = 2.0 * np.pi * ((np.arange(1, N // 2)[:, None] * np.arange(N)[None, :]) % N) / N
    return np.abs(np.cos(ang)), np.abs(np.sin(ang))


def inverse_terms(S, w):
    """[F, n_fft]: sum |t_i| of the inverse half for the spectrum S [F, bins] it transforms:
    w[n] / N (|Re S_0| + |Re S_{N/2}| + 2 sum_{0 < k < N/2} (|Re S_k cos(2 pi k n / N)| + |Im S_k sin(2 pi k n / N)|))."""
    S = np.asarray(S, np.complex128)
    N = len(w)
    c, s = _abs_twiddles(N)
    t = np.abs(S[:, :1].real) + np.abs(S[:, -1:].real) + 2.0 * (np.abs(S[:, 1:-1].real) @ c + np.abs(S[:, 1:-1].imag) @ s)
    return t / N * np.abs(w)[None, :]


def inverse_bound(S, w):
    """[F, n_fft]: bound on the frames a launch writes against frames(S) for the spectrum S the launch projected."""
    return (chain_of(len(w)) + 8) * U * inverse_terms(S, w)


def inverse_of_bound(dS, w):
    """[F, n_fft]: a per-bin bound |dS_k| on the spectrum pushed through the inverse map: w[n] / N (d_0 + d_{N/2} + 2 sum d_k)."""
    N = len(w)
    t = (dS[:, 0] + dS[:, -1] + 2.0 * dS[:, 1:-1].sum(axis=1)) / N
    return t[:, None] * np.abs(w)[None, :]


def plain_step_bound(frames_in, amp, w, hop):
    """The plain late-iteration check: (frames_out, bound [F, n_fft]) for one step from frames_in.  The inverse half's own
    bound plus the model of the projection: with e_Z = sqrt(2) forward_bound (both components) and Z the reference's own
    transform, bin k may move by amp_k min(2, e_Z / (|Z_k| - e_Z)); that goes through the inverse map."""
    Z, out = step(frames_in, amp, w, hop)
    eZ = np.sqrt(2.0) * forward_bound(frames_in, w, hop)[:, None]
    gap = np.abs(Z) - eZ
    move = np.where(gap > 0, np.minimum(2.0, eZ / np.where(gap > 0, gap, 1.0)), 2.0)
    moved = inverse_of_bound(amp * move, w)             # ... and the moved spectrum's terms are larger by at most as much
    return out, inverse_bound(project(Z, amp), w) + (1.0 + (chain_of(len(w)) + 8) * U) * moved


PLAIN_CAP = 5e-3        # of the reference frames' peak: cases whose plain_step_bound stays under it take the late plain check


# ------------------------------------------------------------------------------------------ inverse pre-emphasis
def inv_preemphasis(x, coeff):
    """y[n] = x[n] + coeff y[n - 1]  (scipy.signal.lfilter([1], [1, -coeff], x))."""
    y = np.array(x, np.float64)
    for n in range(1, len(y)):
        y[n] += coeff * y[n - 1]
    return y


def inv_preemphasis_bound(x, coeff):
    """[L]: (1 / (1 - |coeff|) + 8) u sum_j |coeff|^j |x[n - j]|: every stored y is a sum whose rounding errors are fed back
    with weights |coeff|^j."""
    return (1.0 / (1.0 - abs(coeff)) + 8) * U * inv_preemphasis(np.abs(x), abs(coeff))


def block_sum_terms(n, threads=PT):
    """Additions into a one-block sum of n values: the per-thread stride count plus the 16 per-wave partials."""
    return -(-n // threads) + 16


def normalize(y, target):
    """y * target / mean|y|; unchanged when target <= 0, when y is empty or all zero."""
    y = np.asarray(y, np.float64)
    tot = np.abs(y).sum()
    return y * (target / (tot / len(y))) if target > 0 and len(y) and tot > 0 else y


def normalize_bound(y, y_bound, target):
    """[L]: bound on the normalised samples.  The scale is target L / tot with tot a block sum of |y|: relative
    (block_sum_terms + 8) u plus the share sum(y_bound) / tot that the samples' own bound moves it; the product adds u."""
    y = np.asarray(y, np.float64)
    tot = np.abs(y).sum()
    if not (target > 0 and len(y) and tot > 0):
        return y_bound
    sc = target * len(y) / tot
    rel = (block_sum_terms(len(y)) + 8) * U + y_bound.sum() / tot
    return sc * y_bound + sc * np.abs(y) * (rel + U)


# ------------------------------------------------------------------------------------------ power -> amplitude
def power_to_amp(P, norm, realse):
    """P [F, bins] -> amplitude [F, bins]: clip at 0, optional P ** realse with the mean kept, 10 ** (0.05 (P / norm - 80))."""
    P = np.maximum(0.0, np.asarray(P, np.float64))
    if realse != 1.0:
        with np.errstate(invalid='ignore', divide='ignore'):
            Q = P ** realse
            P = (P.sum() / Q.sum()) * Q
    return 10.0 ** (0.05 * (P / norm - 80.0))


def power_to_amp_rel_bound(P, norm, realse):
    """[F, bins]: relative bound ln(10) 0.05 e + 4 ulp with e the absolute float32 error of the exponent  v / norm - 80:
    v / norm carries 2 u (reciprocal, product) and, with realse != 1, the gain's two block sums ((block_sum_terms + 8) u
    each, all terms non-negative), powf twice (4 ulp = 8 u each), the division and the product; the subtraction and the
    product with 0.05f round once each at the size of the exponent."""
    P = np.maximum(0.0, np.asarray(P, np.float64))
    g = 2 * U
    if realse != 1.0:
        g += (2 * (block_sum_terms(P.size) + 8) + 8 + 8 + 2) * U
        with np.errstate(invalid='ignore', divide='ignore'):
            Q = P ** realse
            P = (P.sum() / Q.sum()) * Q
    e = np.abs(P / norm) * g + 3 * U * np.abs(P / norm - 80.0)
    return np.log(10.0) * 0.05 * e + 8 * U
