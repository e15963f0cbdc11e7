"""Exemplar conversion on the MI355X: the non-parallel route that needs the phoneme recogniser, a few minutes of any target
speech, no training and no decoder (PPG-based exemplar conversion; kNN-VC, Baas et al. 2023, with posteriorgrams in place of
WavLM features).

The target speaker is a BANK of their own frames, each keyed by the recogniser's posterior; a source frame is replaced by
the mean of the k bank frames whose posteriors are nearest.  The Bhattacharyya coefficient of two posteriors is the dot
product of their square roots; with the roots in 8 bits the search is an int8 matrix product, and its integer arithmetic
makes everything here exact: the device equals the numpy restatement tests/exemplar_ref.py bit for bit.

  key_width(C)                                                          -> 64 or 128
  ppg_keys(ppg, n_frames)                                               -> (key [B, F, Kp] int8, norm [B, F] int32)
  build_bank(ppg, n_frames, stft, mel, mask=None)                       -> Bank
  bank_wav(encoder, wav, lens, cfg_d, mask='energy', wav_sr=None, ...)  -> Bank
  knn_batch(keys, norms, n_frames, bank, k=4, exclude=None, n_splits=0) -> (idx, dist) [B, F, k] int32
  mean_batch(idx, dist, values, d_max=None)                             -> (out [B, F, D], n_used [B, F])

conversion.convert_knn_diff_batch strings them in front of the differential filter.  Definitions: include/vc_hip.h,
"Exemplar conversion"; DESIGN.md section 34.  Every check is made on the host before the first launch; the search and the
mean copy nothing to the host and wait for nothing (build_bank compacts with torch indexing and does wait: a bank is built
once).  All arithmetic runs in csrc/vc_knn.hip.  There is no CPU path.
"""
from collections import namedtuple

import numpy as np

import _vc
import evaluation as ev

MAX_CLASSES = 128
MAX_K = 16
MAX_ROWS = 2 ** 24
MAX_SPLITS = 1024
MAX_DIM = 65536
D_SCALE = 2 * 127 * 127         # dist / D_SCALE approximates the squared Hellinger distance of the two posteriors

Bank = namedtuple('Bank', 'key norm stft mel utt frame rows n_classes')


# ------------------------------------------------------------------------------------------------------------- host checks
def key_width(C):
    """Bytes of a key of C classes: 64 for C <= 64, else 128."""
    C = int(C)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(' - ERROR, key_width: 1 <= C <= {} classes (got {})'.format(MAX_CLASSES, C))
    return 64 if C <= 64 else 128


def _check_counts(n, B, F, what):
    h = np.asarray(n.cpu() if hasattr(n, 'cpu') else n)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > F:
        raise ValueError(' - ERROR, {}: n_frames must be {} integers in [0, {}]'.format(what, B, F))
    return h.astype(np.int32)


def _check_k(k, what):
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(' - ERROR, {}: k must be an integer in [1, {}] (got {!r})'.format(what, MAX_K, k))
    return int(k)


def _check_bank(bank, what):
    if not (isinstance(bank, tuple) and len(bank) == len(Bank._fields)):
        raise ValueError(' - ERROR, {}: bank must be an exemplar.Bank'.format(what))
    key, norm = bank.key, bank.norm
    if getattr(key, 'ndim', 0) != 2 or str(key.dtype) not in ('torch.int8', 'int8') or int(key.shape[1]) not in (64, 128):
        raise ValueError(' - ERROR, {}: bank.key must be int8 [N, 64] or [N, 128]'.format(what))
    N = int(key.shape[0])
    if not 1 <= N <= MAX_ROWS:
        raise ValueError(' - ERROR, {}: a bank holds 1 to 2^24 rows (got {})'.format(what, N))
    if tuple(norm.shape) != (N,) or str(norm.dtype) not in ('torch.int32', 'int32'):
        raise ValueError(' - ERROR, {}: bank.norm must be int32 [{}]'.format(what, N))
    return N, int(key.shape[1])


def _check_exclude(exclude, B, N, what):
    if exclude is None:
        return None
    h = np.asarray(exclude.cpu() if hasattr(exclude, 'cpu') else exclude)
    if h.shape == (2,):
        h = np.broadcast_to(h, (B, 2))
    if h.shape != (B, 2) or h.dtype.kind not in 'iu':
        raise ValueError(' - ERROR, {}: exclude must be [{}, 2] integers (or one pair)'.format(what, B))
    if (h[:, 0] < 0).any() or (h[:, 0] > h[:, 1]).any() or (h[:, 1] > N).any():
        raise ValueError(' - ERROR, {}: every exclude range must be ordered and inside [0, {}]'.format(what, N))
    return np.ascontiguousarray(h, dtype=np.int32)


def _check_d_max(d_max, what):
    if d_max is None:
        return -1
    if int(d_max) != d_max or not 0 <= int(d_max) < 2 ** 31:
        raise ValueError(' - ERROR, {}: d_max must be None or a non-negative integer distance (got {!r})'.format(what, d_max))
    return int(d_max)


def _check_splits(n_splits, what):
    if int(n_splits) != n_splits or not 0 <= int(n_splits) <= MAX_SPLITS:
        raise ValueError(' - ERROR, {}: n_splits must be an integer in [0, {}] (got {!r})'.format(what, MAX_SPLITS, n_splits))
    return int(n_splits)


def _dev(t, dtype):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t))
    return t.to(device='cuda', dtype=dtype).contiguous()


# ---------------------------------------------------------------------------------------------------------------- launches
def _key_launch(ppg, d_nf):
    import torch
    B, F, C = ppg.shape
    Kp = key_width(C)
    key = torch.empty((B, F, Kp), dtype=torch.int8, device=ppg.device)
    norm = torch.empty((B, F), dtype=torch.int32, device=ppg.device)
    _vc.check(_vc.lib().vc_ppg_key_i8(_vc.ptr(ppg), _vc.ptr(d_nf), B, F, C, _vc.ptr(key), _vc.ptr(norm), _vc.current_stream()))
    return key, norm


def workspace_bytes(Mq, N, k, n_splits=0):
    """vc_knn_workspace_bytes: host arithmetic."""
    return int(_vc.lib().vc_knn_workspace_bytes(int(Mq), int(N), int(k), int(n_splits)))


def _knn_launch(keys, norms, d_nf, h_excl, d_excl, bank, k, n_splits, ws=None):
    import torch
    B, F, Kp = keys.shape
    N = bank.key.shape[0]
    if ws is None:
        ws = torch.empty((workspace_bytes(B * F, N, k, n_splits),), dtype=torch.uint8, device=keys.device)
    idx = torch.empty((B, F, k), dtype=torch.int32, device=keys.device)
    dist = torch.empty((B, F, k), dtype=torch.int32, device=keys.device)
    _vc.check(_vc.lib().vc_knn_i8(_vc.ptr(keys), _vc.ptr(norms), _vc.ptr(d_nf), _vc.ptr(h_excl), _vc.ptr(d_excl), B, F,
                                  _vc.ptr(bank.key), _vc.ptr(bank.norm), N, Kp, k, n_splits, _vc.ptr(ws), ws.numel(), _vc.ptr(idx),
                                  _vc.ptr(dist), _vc.current_stream()))
    return idx, dist


def _mean_launch(idx, dist, values, d_max):
    import torch
    B, F, k = idx.shape
    N, D = values.shape
    out = torch.empty((B, F, D), dtype=torch.float32, device=idx.device)
    n_used = torch.empty((B, F), dtype=torch.int32, device=idx.device)
    _vc.check(_vc.lib().vc_knn_mean_f32(_vc.ptr(idx), _vc.ptr(dist), B * F, k, d_max, _vc.ptr(values), N, D, _vc.ptr(out),
                                        _vc.ptr(n_used), _vc.current_stream()))
    return out, n_used


# ------------------------------------------------------------------------------------------------------------ entry points
def ppg_keys(ppg, n_frames):
    """Posteriors [B, F, C] float32 (C <= 128) and n_frames [B] (0 .. F) to keys [B, F, Kp] int8 and norms [B, F] int32; rows
    at or beyond an utterance's frame count hold the zero key and norm 0."""
    import torch
    what = 'ppg_keys'
    B, F, C = ev._check_ppg(ppg, what + ': ppg')
    key_width(C)
    if B * F > MAX_ROWS:
        raise ValueError(' - ERROR, {}: at most 2^24 rows (got {} x {})'.format(what, B, F))
    h_nf = _check_counts(n_frames, B, F, what)
    ev._need_gpu(what)
    return _key_launch(ev._to_device(ppg, torch.float32), ev._upload_lens(h_nf)[0])


def build_bank(ppg, n_frames, stft, mel, mask=None):
    """The bank of B utterances: posteriors [B, F, C], n_frames [B], the front-end's normalised dB spectrum stft [B, F, bins]
    and mel [B, F, n_mels] cut to the same frames, and an optional mask [B, F] (non-zero: keep).  The kept frames among the
    valid ones are compacted in (utterance, frame) order.  Returns Bank(key [N, Kp] int8, norm [N] int32, stft [N, bins], mel
    [N, n_mels], utt [N] int32, frame [N] int32, rows [B, 2] int32 on the host -- utterance b owns the bank rows
    rows[b, 0] .. rows[b, 1] - 1, which is what ``exclude`` takes -- and n_classes).  Torch indexing, and the host waits."""
    import torch
    what = 'build_bank'
    B, F, C = ev._check_ppg(ppg, what + ': ppg')
    key_width(C)
    h_nf = _check_counts(n_frames, B, F, what)
    for t, name in ((stft, 'stft'), (mel, 'mel')):
        if getattr(t, 'ndim', 0) != 3 or tuple(t.shape[:2]) != (B, F) or int(t.shape[2]) < 1 or str(t.dtype) not in ('torch.float32', 'float32'):
            raise ValueError(' - ERROR, {}: {} must be float32 [{}, {}, D]'.format(what, name, B, F))
    if mask is not None and tuple(mask.shape) != (B, F):
        raise ValueError(' - ERROR, {}: mask must be [{}, {}]'.format(what, B, F))
    ev._need_gpu(what)
    ppg, stft, mel = (ev._to_device(t, torch.float32) for t in (ppg, stft, mel))
    d_nf = ev._upload_lens(h_nf)[0]
    key, norm = _key_launch(ppg, d_nf)
    keep = torch.arange(F, device=ppg.device)[None, :] < d_nf[:, None]
    if mask is not None:
        keep &= _dev(mask, torch.uint8) != 0
    utt, frame = (t.to(torch.int32).contiguous() for t in torch.nonzero(keep, as_tuple=True))
    N = int(utt.numel())
    if not 1 <= N <= MAX_ROWS:
        raise ValueError(' - ERROR, {}: the bank keeps {} frames; it needs 1 to 2^24'.format(what, N))
    ends = np.cumsum(keep.sum(1).cpu().numpy())
    rows = np.stack([ends - np.diff(np.concatenate([[0], ends])), ends], 1).astype(np.int32)
    return Bank(key[keep].contiguous(), norm[keep].contiguous(), stft[keep].contiguous(), mel[keep].contiguous(), utt, frame, rows, C)


def bank_wav(encoder, wav, lens, cfg_d, mask='energy', wav_sr=None, res_type='kaiser_best', top_db=40.0, max_gap=20, mask_min_run=0,
             t_e=60, two_pass=True, window_batch=64, ppg=None):
    """The bank of B target RECORDINGS: each goes through the resampler (wav_sr), the front-end, the window tables of
    convert_batch (t_s = 0) and the encoder exactly as a side of evaluation.content_wav_batch does (its _content_side), so
    that bank frame f of an utterance is front-end frame f.  mask: None, or 'energy' -- silence is left out by
    evaluation.activity_batch's energy mask (top_db, max_gap, mask_min_run; the window is cfg_d['win_length']).  ppg
    [B, Fout, C]: posteriors that are already there, instead of running the encoder.  Returns a Bank."""
    import torch
    import audio_lib
    import conversion
    what = 'bank_wav'
    if cfg_d is None:
        raise ValueError(' - ERROR, {}: cfg_d (the data-set configuration) is required'.format(what))
    if (encoder is None) == (ppg is None):
        raise ValueError(' - ERROR, {}: pass exactly one of encoder and ppg'.format(what))
    if mask not in (None, 'energy'):
        raise ValueError(" - ERROR, {}: mask must be None or 'energy', got {!r}".format(what, mask))
    audio_lib._res_params(res_type)
    try:
        a = ev._wav_side(wav, lens, cfg_d, wav_sr, 'wav')
    except ValueError as e:
        raise ValueError(str(e).replace('mcd_wav_batch', what)) from None
    window_batch = int(window_batch)
    if window_batch <= 0:
        raise ValueError(' - ERROR, {}: window_batch must be positive'.format(what))
    plan = conversion.convert_plan(a['h'], cfg_d, 0, t_e, two_pass)
    B = a['B']
    if ppg is not None:
        if ev._check_ppg(ppg, what + ': ppg')[:2] != (B, plan.Fout):
            raise ValueError(' - ERROR, {}: ppg must be [{}, {}, C]'.format(what, B, plan.Fout))
        key_width(ppg.shape[2])
    else:
        key_width(int(encoder.cfg_d['n_output']))
    if mask is not None:
        act = ev._activity_args(mask, top_db, max_gap, mask_min_run, what)
        ev._check_energy(cfg_d['hop_length'], cfg_d['win_length'], a['Fmax'], what)
    h_n = np.minimum(plan.n_out, plan.n_clip)
    ev._need_gpu(what)
    d_in, d_len, d_fr, d_clip, d_win, d_utt, d_true = ev._upload_lens(a['h_in'], a['h'], a['n_frames'], plan.n_clip, plan.win_tab,
                                                                      plan.utt_tab, plan.true_tab)
    d_true = d_true.view(-1, 2)
    if ppg is not None:
        ppg = ev._to_device(ppg, torch.float32)
    x, mel, ppg = ev._content_side(encoder, wav, a, plan, (d_in, d_len, d_clip, d_win.view(-1, 2), d_utt.view(-1, 3), d_true), cfg_d,
                                   res_type, window_batch, ppg)
    stft = conversion.cut_windows(ev._fe_launch(x, d_len, cfg_d)[2], d_true, d_clip, plan.Fout)
    m = None
    if mask is not None:
        full = ev._wav_mask(x.contiguous(), d_len, d_fr, cfg_d, act, None)
        m = torch.zeros((B, plan.Fout), dtype=torch.uint8, device=full.device)
        n = min(plan.Fout, full.shape[1])
        m[:, :n] = full[:, :n]
    return build_bank(ppg, h_n, stft, mel, m)


def knn_batch(keys, norms, n_frames, bank, k=4, exclude=None, n_splits=0):
    """The k nearest bank rows of every query key: keys [B, F, Kp] int8 and norms [B, F] int32 as ppg_keys returns them,
    n_frames [B].  exclude: None, one pair or [B, 2] bank row ranges [lo, hi) that an utterance must not draw from (bank.rows:
    leave-one-out when the bank holds the queries' own recordings).  n_splits: 0, or over how many workgroup columns the
    bank is split (the result does not depend on it).  Returns idx, dist [B, F, k] int32 on the device, ordered by
    (dist, idx); -1 in slots without a candidate and in rows at or beyond n_frames."""
    import torch
    what = 'knn_batch'
    N, Kp = _check_bank(bank, what)
    if getattr(keys, 'ndim', 0) != 3 or str(keys.dtype) not in ('torch.int8', 'int8') or int(keys.shape[2]) != Kp or min(keys.shape) < 1:
        raise ValueError(' - ERROR, {}: keys must be int8 [B, F, {}] like the bank'.format(what, Kp))
    B, F = int(keys.shape[0]), int(keys.shape[1])
    if tuple(norms.shape) != (B, F) or str(norms.dtype) not in ('torch.int32', 'int32'):
        raise ValueError(' - ERROR, {}: norms must be int32 [{}, {}]'.format(what, B, F))
    if B * F > MAX_ROWS:
        raise ValueError(' - ERROR, {}: at most 2^24 query rows (got {} x {})'.format(what, B, F))
    k, n_splits = _check_k(k, what), _check_splits(n_splits, what)
    h_nf = _check_counts(n_frames, B, F, what)
    h_excl = _check_exclude(exclude, B, N, what)
    ev._need_gpu(what)
    if h_excl is None:
        d_nf, d_excl = ev._upload_lens(h_nf)[0], None
    else:
        d_nf, d_excl = ev._upload_lens(h_nf, h_excl)
    bank = bank._replace(key=_dev(bank.key, torch.int8), norm=_dev(bank.norm, torch.int32))
    return _knn_launch(_dev(keys, torch.int8), _dev(norms, torch.int32), d_nf, h_excl, d_excl, bank, k, n_splits)


def mean_batch(idx, dist, values, d_max=None):
    """The mean of the retrieved rows: idx, dist [B, F, k] int32 as knn_batch returns them, values [N, D] float32 (bank.stft,
    bank.mel).  d_max: None, or the largest distance a slot after the first may have (an integer; D_SCALE * h for a squared
    Hellinger distance h).  float32 additions in slot order and one division.  Returns out [B, F, D] float32 (zeros where no
    slot is filled) and n_used [B, F] int32."""
    import torch
    what = 'mean_batch'
    if getattr(idx, 'ndim', 0) != 3 or min(idx.shape) < 1 or tuple(dist.shape) != tuple(idx.shape):
        raise ValueError(' - ERROR, {}: idx and dist must be [B, F, k], alike'.format(what))
    for t, name in ((idx, 'idx'), (dist, 'dist')):
        if str(t.dtype) not in ('torch.int32', 'int32'):
            raise ValueError(' - ERROR, {}: {} must be int32, got {}'.format(what, name, t.dtype))
    _check_k(idx.shape[2], what)
    if int(idx.shape[0]) * int(idx.shape[1]) > MAX_ROWS:
        raise ValueError(' - ERROR, {}: at most 2^24 query rows'.format(what))
    if getattr(values, 'ndim', 0) != 2 or str(values.dtype) not in ('torch.float32', 'float32'):
        raise ValueError(' - ERROR, {}: values must be float32 [N, D]'.format(what))
    if not (1 <= int(values.shape[0]) <= MAX_ROWS and 1 <= int(values.shape[1]) <= MAX_DIM):
        raise ValueError(' - ERROR, {}: values must hold 1 to 2^24 rows of 1 to {} columns'.format(what, MAX_DIM))
    d_max = _check_d_max(d_max, what)
    ev._need_gpu(what)
    return _mean_launch(_dev(idx, torch.int32), _dev(dist, torch.int32), _dev(values, torch.float32), d_max)
