"""Float64 reference of the general front-end (csrc/vc_frontend.hip), stage by stage as the device splits the work.

numpy only; nothing of the project and nothing of oracle/ is imported.  A configuration is the keyword dictionary of
``audio_lib.calc_MFCC_input`` (conftest.FE_KW and its variants).

  stage 1  abssum_partials   16 chunk sums of |x| per utterance (only launched with hop > n_fft/2)
  stage 2  stage2            raw power dB, raw mel dB, one record per tile of G frames
  stage 3  stage3            offsets, clamps, floors, min shift, scale, clip, DCT, first coefficient, delta

The amplitude normalisation y *= norm / mean|y| is linear up to the power spectrum, so stage 2 runs on the unscaled signal and
stage 3 adds 20 log10 c to the power dB and 40 log10 c to the mel dB (the mel dB is amplitude_to_db of the mel POWER)."""
import numpy as np

NPART = 16                      # |x| partial sums per utterance
G3 = 32                         # frames per finalize tile
STAT = 8                        # floats per tile record: pmax pmin mmax mmin sum|x| - - -
F32_MAX = float(np.finfo(np.float32).max)
NEUTRAL = (-F32_MAX, F32_MAX, -F32_MAX, F32_MAX, 0.0)
LDS_MAX = 160 * 1024
LDS_OPT_IN = 64 * 1024


def n_fft_of(kw):
    return kw['win_length'] if kw['n_fft'] is None else kw['n_fft']


def tile_frames(n_fft):
    """Frames per stage-2 tile: 16 on the 400-point kernel, 8 on the generic one."""
    return 16 if n_fft == 400 else 8


def num_frames(L, hop):
    return 1 + L // hop


# ------------------------------------------------------------------------------------------ tables
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (m - min_log_hz / f_sp)), f_sp * m)


def mel_matrix(sr, n_fft, n_mels):
    """Slaney mel filters, area-normalised, 0 .. sr/2: [n_mels, 1 + n_fft//2]."""
    nb = 1 + n_fft // 2
    fk = np.linspace(0.0, sr / 2.0, nb)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    w = np.zeros((n_mels, nb))
    for i in range(n_mels):
        lower = (fk - edges[i]) / (edges[i + 1] - edges[i])
        upper = (edges[i + 2] - fk) / (edges[i + 2] - edges[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[i + 2] - edges[i]))
    return w


def dct_matrix(n_mfcc, n_mels):
    """Orthonormal DCT-II rows: [n_mfcc, n_mels]."""
    j = np.arange(n_mels)
    d = np.empty((n_mfcc, n_mels))
    d[0] = 1.0 / np.sqrt(n_mels)
    for i in range(1, n_mfcc):
        d[i] = np.cos(i * (2 * j + 1) * np.pi / (2.0 * n_mels)) * np.sqrt(2.0 / n_mels)
    return d


def window_taps(name, win_length):
    """The periodic window of win_length taps (what the plan is handed): 'hann' or 'hamming'."""
    t = np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return {'hann': 0.5 - 0.5 * t, 'hamming': 0.54 - 0.46 * t}[name]


def padded_window(name, win_length, n_fft):
    w = np.zeros(n_fft)
    lpad = (n_fft - win_length) // 2
    w[lpad:lpad + win_length] = window_taps(name, win_length)
    return w


def sparse_mel(mel):
    """The plan's sparse rows: (start [NM], off [NM + 1], non-zeros, widest row, empty rows).  A row is the contiguous
    range first .. last non-zero; an empty row has start 0 and no taps."""
    start, off = [], [0]
    for row in mel:
        nz = np.nonzero(row)[0]
        start.append(int(nz[0]) if len(nz) else 0)
        off.append(off[-1] + (int(nz[-1] - nz[0]) + 1 if len(nz) else 0))
    cnt = np.diff(off)
    return np.array(start), np.array(off), int(off[-1]), int(cnt.max()), int((cnt == 0).sum())


# ------------------------------------------------------------------------------------------ routing, LDS, workspace
def routing(kw):
    """'fast400' (csrc/vc_frontend400.hip), 'power400' or 'generic' (csrc/vc_frontend.hip)."""
    n_fft = n_fft_of(kw)
    if n_fft != 400:
        return 'generic'
    widest = sparse_mel(mel_matrix(kw['sr'], 400, kw['n_mels']))[3]
    if kw['hop_length'] == 80 and kw['n_mels'] == 80 and kw['n_mfcc'] == 40 and widest <= 14:
        return 'fast400'
    return 'power400'


def fused_abs(kw):
    """True: stage 2 sums |x| itself; False: fe_abssum_kernel runs (with mean_abs_amp_norm != 1)."""
    return kw['hop_length'] <= n_fft_of(kw) // 2


def lds_bytes(kw):
    """The launcher's dynamic-LDS formulas: {'power': bytes, 'finalize': bytes, 'alias': bool}."""
    n_fft, hop, nm, nc = n_fft_of(kw), kw['hop_length'], kw['n_mels'], kw['n_mfcc']
    nb = 1 + n_fft // 2
    nnz = sparse_mel(mel_matrix(kw['sr'], n_fft, nm))[2]
    G = tile_frames(n_fft)
    span_pad = (hop * (G - 1) + n_fft + 3) & ~3
    mel_lds = nnz * 4 + (2 * nm + 1) * 4 + 32 * 4
    alias = False
    if n_fft == 400:
        rows = 16 * 13 * 17
        alias = nnz <= 1024 and 2 * nm + 1 <= 512 and nnz + 2 * nm + 1 + 32 <= rows
        power = (span_pad + 816 + 2 * rows) * 4 if alias else (span_pad + 816 + 2 * rows + 16 * 201 + 1) * 4 + mel_lds
    else:
        power = (span_pad + 3 * n_fft + 8 * nb) * 4 + mel_lds
    nm4 = (nm + 3) & ~3
    finalize = (nc * (nm4 + 4) + (G3 + 2) * (nm4 + nc) + 4 + nm4 + 8) * 4
    return {'power': power, 'finalize': finalize, 'alias': alias}


def align256(v):
    return (v + 255) & ~255


def ws_layout(kw, batch, max_samples):
    """Byte offsets of the workspace sections of a configuration that is not fast400: partials | records | raw mel dB,
    each 256-byte aligned, no counter block.  Returns (o_partial, o_stats, o_mel, total, ntiles, max_frames)."""
    n_fft = n_fft_of(kw)
    mf = 1 + max_samples // kw['hop_length']
    G = tile_frames(n_fft)
    nt = (mf + G - 1) // G
    o_partial = 0
    o_stats = align256(o_partial + batch * NPART * 4)
    o_mel = align256(o_stats + batch * nt * STAT * 4)
    total = align256(o_mel + batch * mf * kw['n_mels'] * 4)
    return o_partial, o_stats, o_mel, total, nt, mf


# ------------------------------------------------------------------------------------------ stage 1
def abssum_partials(x):
    """fe_abssum: 16 sums of |x| over chunks of ceil(L / 16) samples (the last ones may be empty)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    L = len(x)
    chunk = (L + NPART - 1) // NPART
    return np.array([x[c * chunk:min(L, (c + 1) * chunk)].sum() for c in range(NPART)])


# ------------------------------------------------------------------------------------------ stage 2
def frames_of(x, kw):
    """Pre-emphasis of the unscaled signal, reflect pad of n_fft/2, window: [F, n_fft] float64."""
    x = np.asarray(x, dtype=np.float64)
    n_fft, hop = n_fft_of(kw), kw['hop_length']
    y = x.copy()
    if kw['pre_emphasis'] != 0.0:
        y[1:] -= kw['pre_emphasis'] * x[:-1]
    yp = np.pad(y, n_fft // 2, mode='reflect')
    F = num_frames(len(x), hop)
    idx = hop * np.arange(F)[:, None] + np.arange(n_fft)[None, :]
    return yp[idx] * padded_window(kw['window'], kw['win_length'], n_fft)[None, :]


def tile_records(pow_raw, mel_raw, asum_tiles, G, ntiles):
    """[ntiles, 5] records: max and min of both arrays over each tile's valid frames and the tile's sum|x|; the neutral
    record for tiles at or beyond F."""
    F = pow_raw.shape[0]
    rec = np.tile(np.array(NEUTRAL), (ntiles, 1))
    for t in range((F + G - 1) // G):
        p, m = pow_raw[t * G:(t + 1) * G], mel_raw[t * G:(t + 1) * G]
        rec[t] = (p.max(), p.min(), m.max(), m.min(), asum_tiles[t])
    return rec


def stage2(x, kw, ntiles=None):
    """x: one utterance, unscaled.  Returns (pow_raw [F, NB], mel_raw [F, NM], records [ntiles, 5])."""
    x = np.asarray(x, dtype=np.float64)
    n_fft, hop, L = n_fft_of(kw), kw['hop_length'], len(x)
    G = tile_frames(n_fft)
    S = np.fft.rfft(frames_of(x, kw), axis=1)
    P = S.real ** 2 + S.imag ** 2
    pow_raw = 10.0 * np.log10(np.maximum(1e-30, P))
    M = P @ mel_matrix(kw['sr'], n_fft, kw['n_mels']).T
    mel_raw = 20.0 * np.log10(np.maximum(1e-18, np.abs(M)))
    F = P.shape[0]
    nt_own = (F + G - 1) // G
    ax = np.abs(x)
    asum = [ax[t * G * hop:min((t + 1) * G * hop, L)].sum() for t in range(nt_own)]
    return pow_raw, mel_raw, tile_records(pow_raw, mel_raw, asum, G, nt_own if ntiles is None else ntiles)


# ------------------------------------------------------------------------------------------ stage 3
def stage3(pow_raw, mel_raw, records, partials, L, kw):
    """Finalize of one utterance from what stage 2 (and stage 1) left: raw dB arrays [F, .], tile records (only the first
    ceil(F / G) are read), the 16 partials (read instead of the records' sums when stage 1 ran).
    Returns (mfcc [F, NC or 2 NC], mel [F, NM], pow [F, NB]) float64."""
    n_fft = n_fft_of(kw)
    G = tile_frames(n_fft)
    F = pow_raw.shape[0]
    rec = np.asarray(records, dtype=np.float64)[:(F + G - 1) // G]
    pmax, pmin, mmax, mmin = rec[:, 0].max(), rec[:, 1].min(), rec[:, 2].max(), rec[:, 3].min()
    offp = 0.0
    if kw['mean_abs_amp_norm'] != 1.0:
        asum = rec[:, 4].sum() if fused_abs(kw) else float(np.sum(partials))
        c = kw['mean_abs_amp_norm'] / (asum / L)
        offp = 20.0 * np.log10(c)
    offm = 2.0 * offp
    pmax, pmin = max(pmax + offp, -100.0), max(pmin + offp, -100.0)
    mmax, mmin = max(mmax + offm, -100.0), max(mmin + offm, -100.0)
    pfloor, mfloor = max(pmax - 80.0, -100.0), max(mmax - 80.0, -100.0)
    pmin_c, mmin_c = max(pmin, pfloor), max(mmin, mfloor)

    p = np.maximum(pow_raw + offp, pfloor)
    if kw['P_dB_norm_factor'] != 1.0:
        p = kw['P_dB_norm_factor'] * (p - pmin_c)
    mc = np.maximum(mel_raw + offm, mfloor)
    m = mc
    if kw['M_dB_norm_factor'] != 1.0:
        m = kw['M_dB_norm_factor'] * (mc - mmin_c)
    c = mc @ dct_matrix(kw['n_mfcc'], kw['n_mels']).T
    if kw['mfcc_normaleze_first_mfcc']:
        c[:, 0] -= c[0, 0]
    if kw['mfcc_norm_factor'] != 1.0:
        c = kw['mfcc_norm_factor'] * c
    if kw['calc_mfcc_derivate']:
        d = np.zeros_like(c)
        d[1:-1] = 2.0 * (c[2:] - c[:-2])
        c = np.concatenate([c, d], axis=1)
    if kw['clip_output']:
        c, m, p = (np.clip(v, -1.0, 1.0) for v in (c, m, p))
    return c, m, p


def features(x, kw):
    """All stages of one utterance: (mfcc, mel, pow) float64."""
    pow_raw, mel_raw, rec = stage2(x, kw)
    return stage3(pow_raw, mel_raw, rec, abssum_partials(x), len(x), kw)


def floors(pow_raw, mel_raw):
    """The lowest raw values that can reach an output, whatever the flags: 80 dB below the utterance's maxima."""
    return pow_raw.max() - 80.0, mel_raw.max() - 80.0


# ------------------------------------------------------------------------------------------ float32 model of stage 2
def stage2_f32_sequential(x, kw, max_chunk=1 << 23):
    """A float32 restatement of stage 2's transform at its most pessimistic: float32 samples, window and twiddles, every
    product rounded, one sequential float32 sum per bin (cumsum).  Returns (pow_raw, mel_raw) float64 dB of float32 numbers."""
    n_fft = n_fft_of(kw)
    nb = 1 + n_fft // 2
    x = np.asarray(x, dtype=np.float32)
    y = x.copy()
    if kw['pre_emphasis'] != 0.0:
        y[1:] = x[1:] - np.float32(kw['pre_emphasis']) * x[:-1]
    yp = np.pad(y, n_fft // 2, mode='reflect')
    F = num_frames(len(x), kw['hop_length'])
    idx = kw['hop_length'] * np.arange(F)[:, None] + np.arange(n_fft)[None, :]
    fr = yp[idx] * padded_window(kw['window'], kw['win_length'], n_fft).astype(np.float32)[None, :]
    ang = -2.0 * np.pi * ((np.arange(nb)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    tc, ts = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    P = np.empty((F, nb), np.float32)
    step = max(1, max_chunk // (nb * n_fft))
    for f0 in range(0, F, step):
        v = fr[f0:f0 + step, None, :]
        re = np.cumsum(v * tc[None], axis=2, dtype=np.float32)[:, :, -1]
        im = np.cumsum(v * ts[None], axis=2, dtype=np.float32)[:, :, -1]
        P[f0:f0 + step] = re * re + im * im
    mel32 = mel_matrix(kw['sr'], n_fft, kw['n_mels']).astype(np.float32)
    M = np.cumsum(P[:, None, :] * mel32[None], axis=2, dtype=np.float32)[:, :, -1]
    pow_raw = 10.0 * np.log10(np.maximum(1e-30, P.astype(np.float64)))
    mel_raw = 20.0 * np.log10(np.maximum(1e-18, np.abs(M.astype(np.float64))))
    return pow_raw, mel_raw
