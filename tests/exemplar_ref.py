"""Host restatement of exemplar conversion (include/vc_hip.h, "Exemplar conversion"), in the order the
header writes out: the int8 keys of posteriors, the exact k-nearest-neighbour selection by (distance, row) and the mean of
the retrieved rows -- every one bit for bit what the device returns, since the arithmetic is integer (and, for the mean, a
fixed order of float32 additions and one division).  Then the float64 Hellinger search the quantisation is judged against,
and the corpora of the method's own checks.  Plain numpy (scipy only for the vowels' resonators).  Nothing here is fitted to
a device result.
"""
import numpy as np

import align_ref
import diff_ref
import mapping_ref

MAX_K = 16
D_SCALE = 2 * 127 * 127
BARRED = np.int64(1) << 60          # above every packed (d << 25) | j: d < 2^23, j < 2^25


# ------------------------------------------------------------------------------------------------------------------- keys
def key_width(C):
    assert 1 <= C <= 128
    return 64 if C <= 64 else 128


def keys(ppg, n_frames=None):
    """ppg [..., F, C] float32 -> (key [..., F, Kp] int8, norm [..., F] int32).  n_frames [...]: rows at or beyond it are zero."""
    p = np.asarray(ppg, np.float32)
    C = p.shape[-1]
    Kp = key_width(C)
    pos = p > np.float32(0)                                             # (a NaN compares false)
    with np.errstate(invalid='ignore'):
        root = np.sqrt(np.where(pos, p, np.float32(0)))                 # correctly rounded float32
        q = np.minimum(np.rint(np.float32(127.0) * root), np.float32(127.0))    # one float32 product, half to even
    q = np.where(pos, q, np.float32(0)).astype(np.int32)
    if n_frames is not None:
        live = np.arange(p.shape[-2]) < np.asarray(n_frames)[..., None]
        q = q * live[..., None]
    key = np.zeros(p.shape[:-1] + (Kp,), np.int8)
    key[..., :C] = q
    return key, (q * q).sum(-1).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------- search
def distances(qkey, qnorm, bkey, bnorm):
    """d [Mq, N] int64.  The integer products run through a float64 matmul: exact at these magnitudes (below 2^22)."""
    dot = np.rint(np.asarray(qkey, np.float64) @ np.asarray(bkey, np.float64).T).astype(np.int64)
    return np.asarray(qnorm, np.int64)[:, None] + np.asarray(bnorm, np.int64)[None, :] - 2 * dot


def select(d, k, lo=0, hi=0, cols=None):
    """The first k of the columns of d [M, n] outside [lo, hi) by (d, column): (idx, dist) [M, k] int32, -1 without a
    candidate.  cols: the columns' bank rows when d holds a slice of the bank (ascending); lo, hi scalars or [M]."""
    M, n = d.shape
    j = np.arange(n, dtype=np.int64) if cols is None else np.asarray(cols, np.int64)
    c = d.astype(np.int64) * (1 << 25) + j[None, :]
    lo, hi = np.broadcast_to(np.asarray(lo), (M,)), np.broadcast_to(np.asarray(hi), (M,))
    c = np.where((j[None, :] >= lo[:, None]) & (j[None, :] < hi[:, None]), BARRED, c)
    if n < k:
        c = np.concatenate([c, np.full((M, k - n), BARRED)], 1)
    c = np.sort(c, axis=1)[:, :k]
    ok = c < BARRED
    return np.where(ok, c & ((1 << 25) - 1), -1).astype(np.int32), np.where(ok, c >> 25, -1).astype(np.int32)


def knn(qkey, qnorm, n_frames, bkey, bnorm, k, excl=None, chunk=4096):
    """qkey [B, F, Kp], qnorm [B, F], n_frames [B], bank [N, Kp] / [N], excl None or [B, 2] -> idx, dist [B, F, k] int32."""
    B, F, _ = qkey.shape
    idx, dist = np.full((B, F, k), -1, np.int32), np.full((B, F, k), -1, np.int32)
    for b in range(B):
        n = min(max(int(n_frames[b]), 0), F)
        lo, hi = (0, 0) if excl is None else (int(excl[b][0]), int(excl[b][1]))
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            idx[b, s:e], dist[b, s:e] = select(distances(qkey[b, s:e], qnorm[b, s:e], bkey, bnorm), k, lo, hi)
    return idx, dist


def merge(parts, k):
    """The first k by (d, j) of several (idx, dist) lists [M, k_i] with -1 for empty slots."""
    idx, dist = np.concatenate([p[0] for p in parts], 1).astype(np.int64), np.concatenate([p[1] for p in parts], 1).astype(np.int64)
    c = np.where(idx >= 0, dist * (1 << 25) + idx, BARRED)
    if c.shape[1] < k:
        c = np.concatenate([c, np.full((c.shape[0], k - c.shape[1]), BARRED)], 1)
    c = np.sort(c, axis=1)[:, :k]
    ok = c < BARRED
    return np.where(ok, c & ((1 << 25) - 1), -1).astype(np.int32), np.where(ok, c >> 25, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- mean
def mean(idx, dist, values, d_max=-1):
    """idx, dist [..., k] int32, values [N, D] float32 -> (out [..., D] float32, n_used [...] int32)."""
    V = np.asarray(values, np.float32)
    N, D = V.shape
    shape = idx.shape[:-1]
    idx, dist = idx.reshape(-1, idx.shape[-1]), dist.reshape(-1, idx.shape[-1])
    k = idx.shape[1]
    ok = (idx >= 0) & (idx < N) & ((np.arange(k)[None, :] == 0) | (d_max < 0) | (dist <= d_max))
    alive = np.cumprod(ok, axis=1).astype(bool)                         # the list ends at the first slot that fails
    n = alive.sum(1).astype(np.int32)
    s = np.zeros((len(idx), D), np.float32)
    for i in range(k):
        r = np.nonzero(alive[:, i])[0]
        s[r] = V[idx[r, i]] if i == 0 else (s[r] + V[idx[r, i]]).astype(np.float32)
    has = n > 0
    s[has] = (s[has] / n[has].astype(np.float32)[:, None]).astype(np.float32)
    return s.reshape(shape + (D,)), n.reshape(shape)


# ------------------------------------------------------------------------------------------- what quantisation costs
def hellinger2(p, q):
    """1 - sum_c sqrt(p_c q_c) [M, N] in float64."""
    return 1.0 - np.sqrt(np.asarray(p, np.float64)) @ np.sqrt(np.asarray(q, np.float64)).T


def peaky_posteriors(n, C=61, seed=0, alpha=0.3, lo=0.5, hi=0.97):
    """n independent peaky posteriors: a dominant class at lo .. hi, the rest spread by a sparse Dirichlet(alpha) draw.
    (A first corpus drew every frame from one of 400 jittered prototypes: about fifty bank frames then lie within the
    quantisation step of each query's nearest one, and WHICH of them is nearest in float64 is not a property a quantised
    search can keep -- containment was 0.95 while the mean distance stayed within 0.3 %.  The condition was kept and the
    corpus changed to this one, which is also the kind the figures in DESIGN.md section 34 were first taken on.)"""
    rng = np.random.RandomState(seed)
    peak = rng.uniform(lo, hi, n)
    p = (1.0 - peak)[:, None] * rng.dirichlet(np.full(C, alpha), n)
    p[np.arange(n), rng.randint(0, C, n)] += peak
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def fidelity(n_query=2000, n_bank=20000, C=61, k=8, seed=0):
    """The quantised search against the float64 Hellinger search on peaky_posteriors: (share of queries whose float64
    nearest neighbour is among the quantised first k, mean float64 Hellinger^2 of the quantised search's neighbours, of the
    exact search's, share of queries with a tie inside their first k + 1)."""
    q, b = peaky_posteriors(n_query, C, seed), peaky_posteriors(n_bank, C, seed + 1)
    (qk, qn), (bk, bn) = keys(q), keys(b)
    idx, dist = select(distances(qk, qn, bk, bn), k + 1)
    H = hellinger2(q, b)
    exact = np.argsort(H, axis=1, kind='stable')[:, :k]
    contained = float((idx[:, :k] == exact[:, :1]).any(1).mean())
    rows = np.arange(n_query)[:, None]
    return contained, float(H[rows, idx[:, :k]].mean()), float(H[rows, exact].mean()), float((np.diff(dist, axis=1) == 0).any(1).mean())


# ------------------------------------------------------------------------------------------------- the regression corpus
def regression_corpus(noise, n_classes=21, dim=24, n_bank_utts=16, n_seg=30, seed=0):
    """Two "speakers", an envelope [dim] per class and speaker.  An utterance is a random sequence of n_seg segments of 3
    to 8 frames; its posteriors are align_ref.synthetic_posteriors at ``noise``, its spectrum the speaker's envelopes mixed
    by the noise-free smoothed segmentation.  Returns a dict: the source's posteriors, its own spectrum and the target's
    trajectory for the same segmentation; the bank's posteriors and spectra (n_bank_utts utterances of the target)."""
    rng = np.random.RandomState(1000 + seed)
    env = rng.uniform(0.1, 0.9, (2, n_classes, dim))

    def utterance(s, who):
        labs, lens = rng.randint(0, n_classes, n_seg), rng.randint(3, 9, n_seg)
        post = align_ref.synthetic_posteriors(labs, lens, n_classes, seed=s, noise=noise)
        mix = align_ref.synthetic_posteriors(labs, lens, n_classes, seed=s, peak=1.0, noise=0.0).astype(np.float64)
        return post, mix @ env[who], mix @ env[1]

    q_post, q_src, q_tgt = utterance(0, 0)
    bank = [utterance(1 + u, 1) for u in range(n_bank_utts)]
    return dict(ppg=q_post, src=q_src.astype(np.float32), tgt=q_tgt.astype(np.float32),
                bank_ppg=[u[0] for u in bank], bank_spec=[u[1].astype(np.float32) for u in bank], n_classes=n_classes)


def regression_figures(c, k=4, d_max=-1):
    """(rms of the retrieved spectrum to the target's trajectory, rms of the source's own spectrum to it, idx, dist, out)."""
    (qk, qn), (bk, bn) = keys(c['ppg']), keys(np.concatenate(c['bank_ppg']))
    idx, dist = select(distances(qk, qn, bk, bn), k)
    out, _ = mean(idx, dist, np.concatenate(c['bank_spec']), d_max)
    rms = lambda a, b: float(np.sqrt(((a.astype(np.float64) - b) ** 2).mean()))
    return rms(out, c['tgt']), rms(c['src'], c['tgt']), idx, dist, out


# ------------------------------------------------------------------------------------------------------ the vowel corpus
VOWEL_CLASSES = 8                    # the four vowels of mapping_ref.FORMANTS are classes 0 .. 3 of 8
TARGET_SCALE = 1.17


def vowel_corpus(n_bank=3, seed=11, hop=80, sr=16000, noise=0.02):
    """A source sentence of four vowels (mapping_ref.sentence), the target speaker's rendition of it (formants x 1.17, same
    order and durations) and n_bank other sentences of the target with their own orders and durations, all on one pulse
    train; with every waveform its posteriors from the known segmentation (align_ref.synthetic_posteriors over
    VOWEL_CLASSES classes, one row per front-end frame 1 + len // hop).  Returns a dict of float32 arrays and lists."""
    rng = np.random.RandomState(seed)

    def one(order, dur, scale, s):
        w = mapping_ref.sentence(order, dur, scale, sr=sr).astype(np.float32)
        F = 1 + len(w) // hop
        ends = np.minimum(np.rint(np.cumsum([int(round(d * sr)) for d in dur]) / float(hop)).astype(int), F)
        ends[-1] = F
        lens = np.diff(np.concatenate([[0], ends]))
        return w, align_ref.synthetic_posteriors(order, lens, VOWEL_CLASSES, seed=s, noise=noise)

    order, dur = rng.permutation(4), rng.uniform(0.2, 0.3, 4)
    src, src_ppg = one(order, dur, 1.0, 0)
    tgt, _ = one(order, dur, TARGET_SCALE, 0)
    bank = [one(rng.permutation(4), rng.uniform(0.2, 0.3, 4), TARGET_SCALE, 1 + u) for u in range(n_bank)]
    return dict(src=src, src_ppg=src_ppg, tgt=tgt, bank_wav=[b[0] for b in bank], bank_ppg=[b[1] for b in bank])


def vowel_restatement(corpus, cfg, k=4, n_use=None):
    """The conversion of the vowel corpus in numpy: the oracle's front-end for the bank's and the source's normalised dB
    spectra, keys, search and mean as above, diff_ref's float64 gain and filter.  Returns (filtered waveform, the smoothed
    log-spectral distance of the source to the target's rendition, that of the output, stft_pred)."""
    from oracle import frontend_oracle as fo
    import vocoder_kernels_ref as vr
    fe = {key: cfg[key] for key in ('pre_emphasis', 'hop_length', 'win_length', 'n_mels', 'n_mfcc', 'n_fft', 'window',
                                    'mfcc_normaleze_first_mfcc', 'mfcc_norm_factor', 'calc_mfcc_derivate', 'M_dB_norm_factor',
                                    'P_dB_norm_factor', 'mean_abs_amp_norm', 'clip_output')}
    spec = lambda w: np.asarray(fo.calc_MFCC_input(w, sr=cfg['sample_rate'], **fe)[2], np.float32)
    hop = cfg['hop_length']
    bank_spec = np.concatenate([spec(w) for w in corpus['bank_wav']])
    src_spec = spec(corpus['src'])
    F = len(src_spec) if n_use is None else n_use
    (qk, qn), (bk, bn) = keys(corpus['src_ppg'][:F]), keys(np.concatenate(corpus['bank_ppg']))
    assert len(bk) == len(bank_spec)
    idx, dist = select(distances(qk, qn, bk, bn), k)
    pred, _ = mean(idx, dist, bank_spec)
    taps = diff_ref.smoothing_taps(8)
    G = diff_ref.gain(pred[None], src_spec[None, :F], [F], cfg['P_dB_norm_factor'], taps)[0]
    win = vr.device_window(vr.padded_window(cfg['win_length'], cfg['win_length']))
    y = diff_ref.stft_filter(corpus['src'].astype(np.float64), G, win, hop, F)
    n = len(y)
    lsd = lambda a: diff_ref.log_spectral_distance(a[:n], corpus['tgt'][:n].astype(np.float64), win, hop, taps)
    return y, lsd(corpus['src'].astype(np.float64)), lsd(y), pred
