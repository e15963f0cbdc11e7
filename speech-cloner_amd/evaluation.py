"""Scoring a conversion on the MI355X: mel-cepstral distortion (MCD, dB) along a dynamic-time-warping (DTW) path, and the
F0 error and voiced / unvoiced error along the same path.

The reference judges a conversion by eye and by ear (test.py:338-343, ``show_spec_comp`` and ``sd.play``).  Its TEST 3
(test.py:379-413) converts CMU-ARCTIC speaker ``rms``, sentence ``a0407``, to ``bdl``; ``bdl``'s own recording of that
sentence exists and has another length, and the usual number for such a pair is the MCD along the DTW path between the
two.  The same number, frame by frame (``align='frame'``), compares two conversions of one input: what ``mxfp8`` or
32 iterations of fast Griffin-Lim cost.

  mel_cepstra(mel [B, F, n_mels]) -> c [B, F, n_coef]           c = Dct[first_coef : first_coef + n_coef] @ mel
  dtw_batch(ca, cb, len_a, len_b, band, return_path)            -> (total [B], path_len [B], mcd [B], path | None)
  mcd_batch(mel_a, mel_b, len_a, len_b, cfg_d, ...)             the two above in one; mel as convert_batch returns it
  mcd_wav_batch(wav_a, lens_a, wav_b, lens_b, cfg_d, ...)       resampler and front-end on both sides first
  f0_batch(wav, lens, sr, hop_length, ...)                      -> (f0 [B, F] Hz, 0 = unvoiced; aperiodicity; n_frames): YIN
  f0_candidates_batch(wav, lens, sr, hop_length, ..., n_cand, ceiling)   -> up to n_cand F0 candidates per frame (f0, pitch, cost, n)
  f0_viterbi_batch(pitch, cost, n, lens, unvoiced_cost, jump_cost, switch_cost, f0)   -> the cheapest path through them (state, total, f0)
  f0_track_batch(wav, lens, sr, hop_length, ..., jump_cost, switch_cost, n_cand)      the two above in one; drops in for f0_batch
  f0_metrics_batch(f0_a, f0_b, len_a, len_b, path, path_len)    voicing error, F0 RMSE (cents, Hz), log-F0 correlation
  score_wav_batch(wav_a, lens_a, wav_b, lens_b, cfg_d, ...)     MCD and the F0 figures along one DTW path in one call
  activity_batch(wav, lens, hop_length, frame_length, mode, ...) -> speech-activity mask, frame list, intervals, frame energy
  compact_batch(x [B, F, C], index, n_kept)                     the rows a frame list names, zeros beyond
  ppg_metrics_batch(ppg_a, ppg_b, len_a, len_b, path, path_len, class_map)   arg-max agreement and Jensen-Shannon divergence (bits) along the cells
  phn_segments_batch(ppg [B, F, C], lens, class_map, min_run)   -> the phoneme sequence: labels, start, end [B, F], n_seg [B]
  edit_distance_batch(seq_a, seq_b, n_a, n_b)                   -> dist, n_match, n_sub, n_del, n_ins, per = dist / n_a
  content_batch(ppg_a, ppg_b, len_a, len_b, ...)                the three above in one (mask_a, mask_b as in mcd_batch)
  content_wav_batch(encoder, wav_a, lens_a, wav_b, lens_b, cfg_d, ...)   resampler, front-end, convert_batch's windows and the encoder on both sides first
  class_map(names, fold=TIMIT_FOLD_39, drop=...)                the int32 table [C] of the usual 61-to-39 folding (host only)
  stoi_batch(ref, deg, lens, wav_sr, extended, ...)             STOI / ESTOI of a TIME-ALIGNED pair -> (score, n_segments, n_kept, seg)
  si_sdr_batch(ref, deg, lens, zero_mean)                       scale-invariant SDR of such a pair in dB -> (si_sdr, valid)
  stoi_bands(fs, n_fft, n_bands, f_min)                         the one-third-octave band table int32 [n_bands, 2] (host only)

mcd_batch (mask_a, mask_b), mcd_wav_batch and score_wav_batch (mask='energy' | 'voiced' | 'energy+voiced') leave silent
frames out of the DTW, the MCD and the F0 figures; without a mask they are what they were.

Definitions (include/vc_hip.h, "Evaluation"):
  d(i, j) = scale * sqrt(2 * sum_d (ca[i, d] - cb[j, d])^2),  scale = 1 / (4 * M_dB_norm_factor) by default
  D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), ties in that order;  mcd = D(end) / path length

Lengths are host integers.  Every check is made on the host before the first launch; after that nothing is copied to
the host and the host waits for nothing.  All arithmetic runs in csrc/vc_dtw.hip, csrc/vc_f0.hip (the pitch tracker
and its figures), csrc/vc_f0_track.hip (the Viterbi decoding of F0 candidates, section 19), csrc/vc_activity.hip (the masks) and csrc/vc_content.hip (the content scores,
DESIGN.md section 17) and csrc/vc_stoi.hip (the intelligibility scores, section 31); there is no CPU path.  Speaker similarity (GMM-UBM, log-likelihood ratios) lives in speaker.py.
"""
from collections import namedtuple

import numpy as np

import _vc

MAX_FRAMES = 16384          # vc_dtw_f32
MAX_COEF = 32

F0_MAX_LAG = 1022           # vc_f0_yin_f32: one lane per lag
F0_MAX_W = 2048
F0_MAX_HOP = 65536
F0_MAX_SAMPLES = 2 ** 30

_RESULT = namedtuple('mcd', 'total path_len mcd path')
_F0 = namedtuple('f0', 'f0 aperiodicity n_frames')
_F0_CAND = namedtuple('f0_candidates', 'f0 pitch cost n aperiodicity frames')
_F0_PATH = namedtuple('f0_viterbi', 'state total f0')
_F0_TRACK = namedtuple('f0_track', 'f0 aperiodicity n_frames state total')
F0_MAX_CAND = 15            # vc_f0_candidates_f32, vc_f0_viterbi_f32: with the unvoiced state, 16 states
F0_METHODS = ('yin', 'viterbi')
_F0_FIELDS = 'n_cells n_both_voiced n_vuv_mismatch vuv_error f0_rmse_cents f0_rmse_hz logf0_corr'
_F0_METRICS = namedtuple('f0_metrics', _F0_FIELDS)
_SCORE = namedtuple('score', 'mcd total path_len path ' + _F0_FIELDS + ' f0_a f0_b n_active_a n_active_b mask_a mask_b')
_ACTIVITY = namedtuple('activity', 'mask index n_active n_kept intervals n_intervals energy n_frames')
_COMPACT = namedtuple('compact', 'index n_active n_kept intervals n_intervals')
_MODES = {'energy': 1, 'voiced': 2, 'energy+voiced': 3}         # vc_activity_mask
ACT_MAX_W = 8192            # vc_frame_energy_f32
ACT_MAX_COLS = 4096         # vc_compact_rows_f32
_DCT = {}


def dct_rows(n_mels, n_coef=24, first_coef=1):
    """Rows first_coef .. first_coef + n_coef - 1 of the orthonormal DCT-II over n_mels points, float32 [n_coef, n_mels]:
    audio_lib.host_tables' table (float64), rounded once.  Host only."""
    import audio_lib
    n_mels, n_coef, first_coef = int(n_mels), int(n_coef), int(first_coef)
    if n_coef < 1 or first_coef < 0 or n_coef + first_coef > n_mels:
        raise ValueError(' - ERROR, mel_cepstra: need n_coef >= 1, first_coef >= 0 and n_coef + first_coef <= n_mels = {} '
                         '(got n_coef {}, first_coef {})'.format(n_mels, n_coef, first_coef))
    if n_coef > MAX_COEF:
        raise ValueError(' - ERROR, mel_cepstra: at most {} coefficients (got {})'.format(MAX_COEF, n_coef))
    dct = audio_lib.host_tables(16000, 2 * n_mels + 2, n_mels, n_coef + first_coef)[1]
    return np.ascontiguousarray(dct[first_coef:first_coef + n_coef].astype(np.float32))


def _check_mel(mel, what):
    import torch
    if getattr(mel, 'ndim', 0) != 3 or min(mel.shape) < 1:
        raise ValueError(' - ERROR, {} must be [B, F, n_mels]'.format(what))
    if torch.is_tensor(mel):
        if mel.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(' - ERROR, {} must be float32 or bfloat16, got {}'.format(what, mel.dtype))
    return tuple(int(v) for v in mel.shape)


def _check_lens(lens, B, Fmax, what):
    h = np.asarray(lens)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 1 or h.max() > Fmax:
        raise ValueError(' - ERROR, {} must be {} integers in [1, {}]'.format(what, B, Fmax))
    return h.astype(np.int64)


def _check_band(band):
    if band is None:
        return -1
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or band < 0 or band >= 2 ** 31:
        raise ValueError(' - ERROR, dtw: band must be None or a non-negative integer number of frames, got {!r}'.format(band))
    return int(band)


def _check_scale(scale):
    s = float(scale)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(' - ERROR, mcd: scale must be finite and positive, got {!r}'.format(scale))
    return s


def _check_pairs(B, Fa, Fb, n_coef, return_path):
    if B > 65535 or Fa > MAX_FRAMES or Fb > MAX_FRAMES:
        raise ValueError(' - ERROR, dtw: at most 65535 pairs of at most {} frames (got {} pairs of {} x {})'.format(MAX_FRAMES, B, Fa, Fb))
    if n_coef > MAX_COEF:
        raise ValueError(' - ERROR, dtw: at most {} coefficients (got {})'.format(MAX_COEF, n_coef))
    if return_path and B * Fa * ((Fb + 15) // 16) * 4 > 2 ** 31:
        raise ValueError(' - ERROR, dtw: the paths of {} pairs of {} x {} frames need more than 2 GiB of predecessor codes; '
                         'score fewer pairs per call'.format(B, Fa, Fb))


def _to_device(t, dtype=None):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device='cuda', dtype=dtype).contiguous()


def _upload_lens(*arrays):
    """One pinned upload of several host int arrays; returns the device slices (no wait)."""
    import torch
    h = torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in arrays])).pin_memory()
    d = h.to('cuda', non_blocking=True)
    offs = np.cumsum([0] + [np.asarray(a).size for a in arrays])
    return [d[offs[i]:offs[i + 1]] for i in range(len(arrays))]


def _dct_device(n_mels, n_coef, first_coef):
    import torch
    key = (n_mels, n_coef, first_coef)
    t = _DCT.get(key)
    if t is None:
        t = _DCT[key] = torch.from_numpy(dct_rows(n_mels, n_coef, first_coef)).pin_memory().to('cuda', non_blocking=True)
    return t


def _cepstra_launch(mel, n_coef, first_coef):
    """mel: cuda, contiguous, float32 or bf16 [B, F, n_mels] -> float32 [B, F, n_coef].  No host check in here."""
    import torch
    B, F, n_mels = mel.shape
    out = torch.empty((B, F, n_coef), dtype=torch.float32, device=mel.device)
    _vc.check(_vc.lib().vc_mel_cepstra(_vc.ptr(mel), _vc.VC_BF16 if mel.dtype == torch.bfloat16 else _vc.VC_F32, B * F, n_mels,
                                       _vc.ptr(_dct_device(n_mels, n_coef, first_coef)), n_coef, _vc.ptr(out), _vc.current_stream()))
    return out


def _dtw_launch(ca, cb, d_la, d_lb, scale, band, return_path):
    import torch
    lib = _vc.lib()
    B, Fa, n_coef = ca.shape
    Fb = cb.shape[1]
    dev = ca.device
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    mcd = torch.empty((B,), dtype=torch.float32, device=dev)
    plen = torch.empty((B,), dtype=torch.int32, device=dev)
    need = lib.vc_dtw_workspace_size(B, Fa, Fb, int(return_path))
    if need == 0:
        raise _vc.VCError('vc_dtw_workspace_size refused {} pairs of {} x {} frames'.format(B, Fa, Fb))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    st = _vc.current_stream()
    _vc.check(lib.vc_dtw_f32(_vc.ptr(ca), _vc.ptr(cb), _vc.ptr(d_la), _vc.ptr(d_lb), B, Fa, Fb, n_coef, scale, band, int(return_path),
                             _vc.ptr(total), _vc.ptr(plen), _vc.ptr(mcd), _vc.ptr(ws), need, st))
    path = None
    if return_path:
        path = torch.empty((B, Fa + Fb - 1, 2), dtype=torch.int32, device=dev)
        _vc.check(lib.vc_dtw_backtrack(_vc.ptr(ws), need, _vc.ptr(d_la), _vc.ptr(d_lb), _vc.ptr(total), _vc.ptr(plen), B, Fa, Fb,
                                       _vc.ptr(path), st))
    return _RESULT(total, plen, mcd, path)


def _frame_launch(ca, cb, d_la, d_lb, scale):
    import torch
    B, Fa, n_coef = ca.shape
    mcd = torch.empty((B,), dtype=torch.float32, device=ca.device)
    _vc.check(_vc.lib().vc_frame_mcd_f32(_vc.ptr(ca), _vc.ptr(cb), _vc.ptr(d_la), _vc.ptr(d_lb), B, Fa, cb.shape[1], n_coef, scale,
                                         _vc.ptr(mcd), _vc.current_stream()))
    return _RESULT(None, None, mcd, None)


def _need_gpu(what):
    import torch
    if not torch.cuda.is_available():
        raise _vc.VCError('{} needs a GPU (no CPU fallback)'.format(what))


def mel_cepstra(mel, n_coef=24, first_coef=1):
    """c[b, f, d] = sum_m Dct[first_coef + d, m] * mel[b, f, m]: float32 [B, F, n_coef] on the device.  mel: float32 or
    bfloat16 [B, F, n_mels], cuda tensor or numpy array (uploaded).  first_coef = 1 leaves out c0, which carries the
    gain: the front-end's amplitude normalisation and per-utterance minimum move c0 alone."""
    B, F, n_mels = _check_mel(mel, 'mel_cepstra: mel')
    dct_rows(n_mels, n_coef, first_coef)                            # validates n_coef / first_coef against n_mels
    if B * F >= 2 ** 31:
        raise ValueError(' - ERROR, mel_cepstra: {} frames exceed int32'.format(B * F))
    _need_gpu('mel_cepstra')
    return _cepstra_launch(_to_device(mel), int(n_coef), int(first_coef))


def dtw_batch(ca, cb, len_a, len_b, band=None, return_path=False, scale=1.0):
    """DTW of B pairs of cepstra over the frame distance scale * sqrt(2 * sum (ca[i] - cb[j])^2) (vc_dtw_f32); ``scale``
    defaults to 1, so ``mcd`` is in dB only when the caller passes the dB scale (mcd_batch does: 25 for the shipped
    M_dB_norm_factor).

    ca [B, Fa_max, n_coef], cb [B, Fb_max, n_coef] float32; len_a, len_b: host integers in [1, F_max].
    band: None, or the half width in frames of the allowed stripe around the straight line from (0, 0) to the end.
    Returns a namedtuple of device tensors: total [B] float32, path_len [B] int32, mcd [B] float32 = total / path_len, and
    path: None, or with return_path int32 [B, Fa_max + Fb_max - 1, 2], the cells (i, j) from (0, 0) to the end, rows from
    path_len on filled with -1."""
    import torch
    for x, what in ((ca, 'ca'), (cb, 'cb')):
        if getattr(x, 'ndim', 0) != 3 or min(x.shape) < 1:
            raise ValueError(' - ERROR, dtw_batch: {} must be [B, F, n_coef]'.format(what))
        if torch.is_tensor(x) and x.dtype != torch.float32:
            raise ValueError(' - ERROR, dtw_batch: {} must be float32'.format(what))
    B, Fa, n_coef = (int(v) for v in ca.shape)
    if int(cb.shape[0]) != B or int(cb.shape[2]) != n_coef:
        raise ValueError(' - ERROR, dtw_batch: ca {} and cb {} must agree in B and n_coef'.format(tuple(ca.shape), tuple(cb.shape)))
    Fb = int(cb.shape[1])
    h_la, h_lb = _check_lens(len_a, B, Fa, 'dtw_batch: len_a'), _check_lens(len_b, B, Fb, 'dtw_batch: len_b')
    band, scale = _check_band(band), _check_scale(scale)
    _check_pairs(B, Fa, Fb, n_coef, return_path)
    _need_gpu('dtw_batch')
    d_la, d_lb = _upload_lens(h_la, h_lb)
    return _dtw_launch(_to_device(ca, torch.float32), _to_device(cb, torch.float32), d_la, d_lb, scale, band, bool(return_path))


def _mcd_args(cfg_d, scale, n_coef, first_coef, align, band, n_mels):
    if align not in ('dtw', 'frame'):
        raise ValueError(" - ERROR, mcd_batch: align must be 'dtw' or 'frame', got {!r}".format(align))
    if scale is None:
        if cfg_d is None:
            raise ValueError(' - ERROR, mcd_batch: pass cfg_d (for M_dB_norm_factor) or scale')
        scale = 1.0 / (4.0 * float(cfg_d['M_dB_norm_factor']))
    dct_rows(n_mels, n_coef, first_coef)                            # validates n_coef / first_coef against n_mels
    return _check_scale(scale), _check_band(band)


def mcd_batch(mel_a, mel_b, len_a, len_b, cfg_d=None, scale=None, n_coef=24, align='dtw', band=None, return_path=False,
              first_coef=1, mask_a=None, mask_b=None):
    """Mel-cepstral distortion in dB of B pairs of mel spectrograms, as convert_batch returns them (mel_pred, mel_true,
    n_frames): mel_a [B, Fa_max, n_mels], mel_b [B, Fb_max, n_mels], float32 or bfloat16; len_a, len_b host integers.

    align='dtw': along the DTW path (``band``, ``return_path`` as in dtw_batch).  align='frame': the mean over the first
    min(len_a, len_b) frames of d(i, i); total, path_len and path are then None.
    scale: None = 1 / (4 * cfg_d['M_dB_norm_factor']), which turns differences of the project's normalised mel into the
    textbook (10 / ln 10) * sqrt(2 * sum (delta mc)^2).
    mask_a [B, Fa_max], mask_b [B, Fb_max]: uint8 or bool, numpy or cuda, 1 = the frame counts (activity_batch's mask; one
    of them None: every frame of that side).  align='dtw': each side is compacted by its own mask and the DTW runs over
    the kept frames; with return_path the path comes back in original frame numbers.  align='frame': one common list, the
    frames where both masks are set, for both sides.  A side without an active frame keeps all its frames."""
    import torch
    Ba, Fa, n_mels = _check_mel(mel_a, 'mcd_batch: mel_a')
    Bb, Fb, n_mels_b = _check_mel(mel_b, 'mcd_batch: mel_b')
    if Ba != Bb or n_mels != n_mels_b:
        raise ValueError(' - ERROR, mcd_batch: mel_a {} and mel_b {} must agree in B and n_mels'.format(tuple(mel_a.shape), tuple(mel_b.shape)))
    n_coef, first_coef = int(n_coef), int(first_coef)
    scale, band = _mcd_args(cfg_d, scale, n_coef, first_coef, align, band, n_mels)
    h_la, h_lb = _check_lens(len_a, Ba, Fa, 'mcd_batch: len_a'), _check_lens(len_b, Ba, Fb, 'mcd_batch: len_b')
    if align == 'dtw':
        _check_pairs(Ba, Fa, Fb, n_coef, return_path)
    elif Ba > 65535:
        raise ValueError(' - ERROR, mcd_batch: at most 65535 pairs')
    masked = mask_a is not None or mask_b is not None
    if masked:
        _check_mask(mask_a, Ba, Fa, 'mcd_batch: mask_a')
        _check_mask(mask_b, Ba, Fb, 'mcd_batch: mask_b')
    _need_gpu('mcd_batch')
    d_la, d_lb = _upload_lens(h_la, h_lb)
    ca = _cepstra_launch(_to_device(mel_a), n_coef, first_coef)
    cb = _cepstra_launch(_to_device(mel_b), n_coef, first_coef)
    if masked:
        ma, mb = _mask_to_device(mask_a, Ba, Fa), _mask_to_device(mask_b, Ba, Fb)
        if align == 'frame':
            return _masked_frame(ca, cb, d_la, d_lb, ma, mb, scale)[0]
        return _masked_dtw(ca, cb, _compact_launch(ma, d_la), _compact_launch(mb, d_lb), scale, band, bool(return_path))
    if align == 'frame':
        return _frame_launch(ca, cb, d_la, d_lb, scale)
    return _dtw_launch(ca, cb, d_la, d_lb, scale, band, bool(return_path))


def _wav_side(wav, lens, cfg_d, wav_sr, what):
    """Host checks of one side of mcd_wav_batch; returns what its launches need."""
    import audio_lib
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, mcd_wav_batch: {} must be [B, Lmax]'.format(what))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    h = np.full((B,), Lmax, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    if h.shape != (B,) or h.min() <= 0 or h.max() > Lmax:
        raise ValueError(' - ERROR, mcd_wav_batch: lens of {} must be [B] with 0 < len <= Lmax'.format(what))
    sr = cfg_d['sample_rate']
    res = wav_sr is not None and audio_lib._ratio(wav_sr, sr) != (1, 1)
    h_in = h
    if res:
        h, Lmax = audio_lib.resample_len(h_in, wav_sr, sr), audio_lib.resample_len(Lmax, wav_sr, sr)
    n_fft = cfg_d['n_fft'] or cfg_d['win_length']
    if h.min() <= n_fft // 2:
        raise ValueError(' - ERROR, mcd_wav_batch: every utterance of {} needs more than n_fft//2 = {} samples at {} Hz'
                         .format(what, n_fft // 2, sr))
    hop = int(cfg_d['hop_length'])
    return dict(B=B, res=res, sr_in=wav_sr, h_in=h_in, h=h, n_frames=1 + h // hop, Fmax=1 + Lmax // hop)


def _wav_at_rate(wav, side, d_in, cfg_d, res_type):
    """One side's waveform on the device at cfg_d['sample_rate'] (through the resampler when its rate differs)."""
    import torch
    import audio_lib
    wav = _to_device(wav, torch.float32)
    if wav.shape[0] == 1:                                           # (the stride of a one-row tensor is arbitrary)
        wav = wav.as_strided(wav.shape, (wav.shape[1], 1))
    if side['res']:
        wav = audio_lib._resample_launch(audio_lib._get_res_plan(side['sr_in'], cfg_d['sample_rate'], res_type), wav, d_in)
    return wav


def _mel_launch(wav, d_len, cfg_d, amp_norm=None):
    return _fe_launch(wav, d_len, cfg_d, amp_norm)[1]


def _fe_launch(wav, d_len, cfg_d, amp_norm=None):
    """The front-end's three outputs (mfcc, mel, stft power) of wav at cfg_d['sample_rate']."""
    import audio_lib
    return audio_lib.calc_MFCC_input_batch(
        wav, d_len, sr=cfg_d['sample_rate'], pre_emphasis=cfg_d['pre_emphasis'], hop_length=cfg_d['hop_length'],
        win_length=cfg_d['win_length'], n_mels=cfg_d['n_mels'], n_mfcc=cfg_d['n_mfcc'], n_fft=cfg_d['n_fft'],
        window=cfg_d['window'], mfcc_normaleze_first_mfcc=cfg_d['mfcc_normaleze_first_mfcc'],
        mfcc_norm_factor=cfg_d['mfcc_norm_factor'], calc_mfcc_derivate=cfg_d['calc_mfcc_derivate'],
        M_dB_norm_factor=cfg_d['M_dB_norm_factor'], P_dB_norm_factor=cfg_d['P_dB_norm_factor'],
        mean_abs_amp_norm=cfg_d['mean_abs_amp_norm'] if amp_norm is None else amp_norm, clip_output=cfg_d['clip_output'])


def _wav_mel(wav, side, d_in, d_len, cfg_d, res_type):
    return _mel_launch(_wav_at_rate(wav, side, d_in, cfg_d, res_type), d_len, cfg_d)


def mcd_wav_batch(wav_a, lens_a, wav_b, lens_b, cfg_d, wav_sr_a=None, wav_sr_b=None, res_type='kaiser_best', scale=None,
                  n_coef=24, align='dtw', band=None, return_path=False, first_coef=1, mask=None, top_db=40.0, max_gap=20,
                  min_run=0, frame_length=512, fmin=60.0, fmax=400.0, threshold=0.15):
    """"Score my conversion against the target's recording" in one call: both sides go through the resampler (when
    their rate wav_sr_a / wav_sr_b differs from cfg_d['sample_rate']) and the front-end, then through mcd_batch.

    wav_a [B, La_max], wav_b [B, Lb_max] float32 (cuda tensor or numpy array); lens_a, lens_b host integers counting
    samples at the side's own rate (None = the whole row); cfg_d: the data-set configuration of test.py.
    Returns mcd_batch's namedtuple; frame counts are 1 + len // hop_length of the (resampled) lengths.
    mask: None, or 'energy', 'voiced', 'energy+voiced' (activity_batch's modes, with top_db, max_gap, min_run): the masks
    are computed from each side's waveform at cfg_d['sample_rate'], after the resampler, the energy over
    cfg_d['win_length'] samples, the voiced modes with the tracker's frame_length, fmin, fmax, threshold; then as
    mcd_batch(mask_a, mask_b).  With a mask the front-end's amplitude normalisation (mean_abs_amp_norm) is taken over the
    samples of the active frames, not over the whole waveform: the front-end floors the mel power, so a gain that depends
    on the share of silence would change the cepstra of the same speech."""
    import audio_lib
    if cfg_d is None:
        raise ValueError(' - ERROR, mcd_wav_batch: cfg_d (the data-set configuration) is required')
    audio_lib._res_params(res_type)
    a = _wav_side(wav_a, lens_a, cfg_d, wav_sr_a, 'wav_a')
    b = _wav_side(wav_b, lens_b, cfg_d, wav_sr_b, 'wav_b')
    if a['B'] != b['B']:
        raise ValueError(' - ERROR, mcd_wav_batch: wav_a and wav_b must hold the same number of utterances')
    n_coef, first_coef = int(n_coef), int(first_coef)
    scale, band = _mcd_args(cfg_d, scale, n_coef, first_coef, align, band, int(cfg_d['n_mels']))
    if align == 'dtw':
        _check_pairs(a['B'], a['Fmax'], b['Fmax'], n_coef, return_path)
    if mask is not None:
        act = _activity_args(mask, top_db, max_gap, min_run, 'mcd_wav_batch')
        _check_energy(cfg_d['hop_length'], cfg_d['win_length'], max(a['Fmax'], b['Fmax']), 'mcd_wav_batch')
        args = _f0_args(cfg_d['sample_rate'], cfg_d['hop_length'], frame_length, fmin, fmax, threshold, 'mcd_wav_batch') if act[0] & 2 else None
    _need_gpu('mcd_wav_batch')
    d_in_a, d_len_a, d_fa, d_in_b, d_len_b, d_fb = _upload_lens(a['h_in'], a['h'], a['n_frames'], b['h_in'], b['h'], b['n_frames'])
    if mask is not None:
        x_a = _wav_at_rate(wav_a, a, d_in_a, cfg_d, res_type).contiguous()
        x_b = _wav_at_rate(wav_b, b, d_in_b, cfg_d, res_type).contiguous()
        ma = _wav_mask(x_a, d_len_a, d_fa, cfg_d, act, _f0_launch(x_a, d_len_a, args)[0] if args else None)
        mb = _wav_mask(x_b, d_len_b, d_fb, cfg_d, act, _f0_launch(x_b, d_len_b, args)[0] if args else None)
        ia, ib = _compact_launch(ma, d_fa), _compact_launch(mb, d_fb)
        ca = _cepstra_launch(_speech_mel(x_a, d_len_a, ma, ia.n_active, cfg_d), n_coef, first_coef)
        cb = _cepstra_launch(_speech_mel(x_b, d_len_b, mb, ib.n_active, cfg_d), n_coef, first_coef)
        if align == 'frame':
            return _masked_frame(ca, cb, d_fa, d_fb, ma, mb, scale)[0]
        return _masked_dtw(ca, cb, ia, ib, scale, band, bool(return_path))
    mel_a = _wav_mel(wav_a, a, d_in_a, d_len_a, cfg_d, res_type)
    mel_b = _wav_mel(wav_b, b, d_in_b, d_len_b, cfg_d, res_type)
    ca = _cepstra_launch(mel_a, n_coef, first_coef)
    cb = _cepstra_launch(mel_b, n_coef, first_coef)
    if align == 'frame':
        return _frame_launch(ca, cb, d_fa, d_fb, scale)
    return _dtw_launch(ca, cb, d_fa, d_fb, scale, band, bool(return_path))


# ------------------------------------------------------------------------------------------------ pitch (csrc/vc_f0.hip)
def _f0_args(sr, hop_length, frame_length, fmin, fmax, threshold, what):
    """Host checks of the tracker's parameters; returns (sr, hop, W, tau_min, tau_max, threshold)."""
    for v, name in ((sr, 'sr'), (hop_length, 'hop_length'), (frame_length, 'frame_length')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(' - ERROR, {}: {} must be a positive integer, got {!r}'.format(what, name, v))
    fmin, fmax, threshold = float(fmin), float(fmax), float(threshold)
    if not (np.isfinite(fmin) and np.isfinite(fmax) and 0.0 < fmin < fmax <= sr):
        raise ValueError(' - ERROR, {}: need 0 < fmin < fmax <= sr (got fmin {}, fmax {}, sr {})'.format(what, fmin, fmax, sr))
    if not (np.isfinite(threshold) and 0.0 < threshold <= 1.0):
        raise ValueError(' - ERROR, {}: threshold must lie in (0, 1], got {!r}'.format(what, threshold))
    tau_min, tau_max = int(np.floor(sr / fmax)), int(np.ceil(sr / fmin))
    if tau_max > F0_MAX_LAG:
        raise ValueError(' - ERROR, {}: fmin {} Hz at {} Hz needs lags up to {}, the kernel holds {} (one lane per lag): raise fmin '
                         'to {:.1f} Hz or more'.format(what, fmin, sr, tau_max, F0_MAX_LAG, sr / float(F0_MAX_LAG)))
    if frame_length > F0_MAX_W or hop_length > F0_MAX_HOP:
        raise ValueError(' - ERROR, {}: frame_length at most {} and hop_length at most {} (got {}, {})'
                         .format(what, F0_MAX_W, F0_MAX_HOP, frame_length, hop_length))
    return int(sr), int(hop_length), int(frame_length), tau_min, tau_max, threshold


def _f0_launch(wav, d_len, args):
    """wav: cuda, contiguous float32 [B, Lmax]; d_len: device int32 [B] or None.  No host check in here."""
    import torch
    sr, hop, W, tau_min, tau_max, thr = args
    B, Lmax = wav.shape
    Fmax = 1 + Lmax // hop
    f0 = torch.empty((B, Fmax), dtype=torch.float32, device=wav.device)
    ap = torch.empty((B, Fmax), dtype=torch.float32, device=wav.device)
    _vc.check(_vc.lib().vc_f0_yin_f32(_vc.ptr(wav), _vc.ptr(d_len), B, Lmax, Lmax, float(sr), hop, W, tau_min, tau_max, thr,
                                      _vc.ptr(f0), _vc.ptr(ap), Fmax, _vc.current_stream()))
    return f0, ap


def _f0_metrics_launch(f0_a, f0_b, d_la, d_lb, path, path_len):
    import torch
    B = f0_a.shape[0]
    counts = torch.empty((B, 3), dtype=torch.int32, device=f0_a.device)
    values = torch.empty((B, 4), dtype=torch.float32, device=f0_a.device)
    _vc.check(_vc.lib().vc_f0_metrics_f32(_vc.ptr(f0_a), _vc.ptr(f0_b), _vc.ptr(d_la), _vc.ptr(d_lb), B, f0_a.shape[1], f0_b.shape[1],
                                          _vc.ptr(path), _vc.ptr(path_len), 0 if path is None else path.shape[1], _vc.ptr(counts),
                                          _vc.ptr(values), _vc.current_stream()))
    return _F0_METRICS(counts[:, 0], counts[:, 1], counts[:, 2], values[:, 0], values[:, 1], values[:, 2], values[:, 3])


def f0_batch(wav, lens=None, sr=16000, hop_length=80, frame_length=512, fmin=60.0, fmax=400.0, threshold=0.15):
    """F0 of B utterances by YIN on the raw waveform (vc_f0_yin_f32; the definition is in include/vc_hip.h).

    wav [B, Lmax] float32 (cuda tensor or numpy array); lens: host integers in [1, Lmax] (None = the whole row).
    Returns a namedtuple: f0 [B, Fmax] float32 in Hz, 0 = unvoiced; aperiodicity [B, Fmax] float32, the minimum of the
    normalised difference over the lag range; n_frames, a list of 1 + len // hop_length per row, the front-end's frame
    count.  Fmax = 1 + Lmax // hop_length; beyond a row's n_frames f0 is 0 and aperiodicity 1.  No smoothing."""
    import torch
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, f0_batch: wav must be [B, Lmax]')
    if torch.is_tensor(wav) and wav.dtype != torch.float32:
        raise ValueError(' - ERROR, f0_batch: wav must be float32, got {}'.format(wav.dtype))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    args = _f0_args(sr, hop_length, frame_length, fmin, fmax, threshold, 'f0_batch')
    h = np.full((B,), Lmax, dtype=np.int64) if lens is None else _check_lens(lens, B, Lmax, 'f0_batch: lens')
    if B > 65535 or Lmax > F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, f0_batch: at most 65535 utterances of at most {} samples (got {} of {})'.format(F0_MAX_SAMPLES, B, Lmax))
    _need_gpu('f0_batch')
    d_len, = _upload_lens(h)
    f0, ap = _f0_launch(_to_device(wav, torch.float32), d_len, args)
    return _F0(f0, ap, [1 + int(n) // args[1] for n in h])


def _track_args(n_cand, ceiling, what):
    if isinstance(n_cand, bool) or not isinstance(n_cand, (int, np.integer)) or not 1 <= n_cand <= F0_MAX_CAND:
        raise ValueError(' - ERROR, {}: n_cand must be an integer in [1, {}], got {!r}'.format(what, F0_MAX_CAND, n_cand))
    ceiling = float(ceiling)
    if not (np.isfinite(ceiling) and ceiling > 0.0):
        raise ValueError(' - ERROR, {}: ceiling must be finite and positive, got {!r}'.format(what, ceiling))
    return int(n_cand), ceiling


def _viterbi_costs(unvoiced_cost, jump_cost, switch_cost, what):
    out = []
    for v, name in ((unvoiced_cost, 'unvoiced_cost'), (jump_cost, 'jump_cost'), (switch_cost, 'switch_cost')):
        v = float(v)
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(' - ERROR, {}: {} must be finite and not negative, got {!r}'.format(what, name, v))
        out.append(v)
    return tuple(out)


def _f0_candidates_launch(wav, d_len, args, n_cand, ceiling):
    """wav: cuda, contiguous float32 [B, Lmax]; d_len: device int32 [B] or None.  No host check in here."""
    import torch
    sr, hop, W, tau_min, tau_max, _ = args
    B, Lmax = wav.shape
    Fmax = 1 + Lmax // hop
    f0, pitch, cost = (torch.empty((B, Fmax, n_cand), dtype=torch.float32, device=wav.device) for _ in range(3))
    n = torch.empty((B, Fmax), dtype=torch.int32, device=wav.device)
    ap = torch.empty((B, Fmax), dtype=torch.float32, device=wav.device)
    _vc.check(_vc.lib().vc_f0_candidates_f32(_vc.ptr(wav), _vc.ptr(d_len), B, Lmax, Lmax, float(sr), hop, W, tau_min, tau_max, ceiling,
                                             n_cand, _vc.ptr(f0), _vc.ptr(pitch), _vc.ptr(cost), _vc.ptr(n), _vc.ptr(ap), Fmax,
                                             _vc.current_stream()))
    return f0, pitch, cost, n, ap


def _f0_viterbi_launch(pitch, cost, n, d_frames, costs, cand_f0):
    """pitch, cost (and cand_f0 or None): cuda, contiguous float32 [B, F, n_cand]; n int32 [B, F]; d_frames device int32
    [B] or None.  No host check in here."""
    import torch
    lib = _vc.lib()
    B, F, n_cand = pitch.shape
    dev = pitch.device
    need = lib.vc_f0_viterbi_workspace_size(B, F, n_cand)
    if need == 0:
        raise _vc.VCError('vc_f0_viterbi_workspace_size refused {} utterances of {} frames with {} candidates'.format(B, F, n_cand))
    ws = torch.empty((need // 8,), dtype=torch.int64, device=dev)
    state = torch.empty((B, F), dtype=torch.int32, device=dev)
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    f0 = None if cand_f0 is None else torch.empty((B, F), dtype=torch.float32, device=dev)
    _vc.check(lib.vc_f0_viterbi_f32(_vc.ptr(pitch), _vc.ptr(cost), _vc.ptr(n), _vc.ptr(d_frames), B, F, n_cand, costs[0], costs[1],
                                    costs[2], _vc.ptr(cand_f0), _vc.ptr(state), _vc.ptr(f0), _vc.ptr(total), _vc.ptr(ws), need,
                                    _vc.current_stream()))
    return state, total, f0


def _f0_track_launch(wav, d_len, d_frames, args, n_cand, ceiling, costs):
    """Both launches of the Viterbi tracker: (f0 [B, Fmax], aperiodicity, state, total).  No host check in here."""
    f0c, pitch, cost, n, ap = _f0_candidates_launch(wav, d_len, args, n_cand, ceiling)
    state, total, f0 = _f0_viterbi_launch(pitch, cost, n, d_frames, costs, f0c)
    return f0, ap, state, total


def _check_wav(wav, what):
    import torch
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    if torch.is_tensor(wav) and wav.dtype != torch.float32:
        raise ValueError(' - ERROR, {}: wav must be float32, got {}'.format(what, wav.dtype))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    if B > 65535 or Lmax > F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most {} samples (got {} of {})'.format(what, F0_MAX_SAMPLES, B, Lmax))
    return B, Lmax


def f0_candidates_batch(wav, lens=None, sr=16000, hop_length=80, frame_length=512, fmin=60.0, fmax=400.0, n_cand=8, ceiling=1.0):
    """Up to n_cand F0 candidates per frame (vc_f0_candidates_f32; the definition is in include/vc_hip.h, "Pitch
    tracking"): the local minima of YIN's d' below ``ceiling``, the n_cand lowest of them, in ascending lag.

    wav, lens, sr, hop_length, frame_length, fmin, fmax as in f0_batch: the frames and d' are f0_batch's.  Returns a
    namedtuple: f0, pitch (= log2 f0), cost (= d' at the lag), each float32 [B, Fmax, n_cand]; n int32 [B, Fmax], the
    number of candidates of a frame (slots from n on hold 0, 0, 1; n = 0 beyond a row's frames and in digital silence);
    aperiodicity [B, Fmax], bit-identical to f0_batch's; frames, the list of frame counts (f0_batch's n_frames)."""
    import torch
    B, Lmax = _check_wav(wav, 'f0_candidates_batch')
    args = _f0_args(sr, hop_length, frame_length, fmin, fmax, 0.5, 'f0_candidates_batch')
    n_cand, ceiling = _track_args(n_cand, ceiling, 'f0_candidates_batch')
    h = np.full((B,), Lmax, dtype=np.int64) if lens is None else _check_lens(lens, B, Lmax, 'f0_candidates_batch: lens')
    _need_gpu('f0_candidates_batch')
    d_len, = _upload_lens(h)
    out = _f0_candidates_launch(_to_device(wav, torch.float32), d_len, args, n_cand, ceiling)
    return _F0_CAND(*out, [1 + int(v) // args[1] for v in h])


def f0_viterbi_batch(pitch, cost, n, lens, unvoiced_cost=0.15, jump_cost=0.5, switch_cost=0.1, f0=None):
    """The cheapest path through a lattice of candidates with an unvoiced state (vc_f0_viterbi_f32).

    pitch, cost float32 [B, F, n_cand] and n int32 [B, F] as f0_candidates_batch returns them (any lattice will do: pitch
    in octaves, cost >= 0, n candidates per frame); lens: host integers in [1, F], the frame counts.  State 0 (unvoiced)
    costs unvoiced_cost per frame, a candidate its cost; moving between unvoiced and voiced costs switch_cost, between
    two candidates jump_cost per octave.  Returns a namedtuple: state int32 [B, F] (0 unvoiced, k candidate k - 1, -1
    beyond a row's frames), total float32 [B] (the path's cost), and f0 [B, F] (0 where unvoiced) when given the
    candidates' f0 [B, F, n_cand], else None."""
    import torch
    for t, name in ((pitch, 'pitch'), (cost, 'cost')) + (((f0, 'f0'),) if f0 is not None else ()):
        if getattr(t, 'ndim', 0) != 3 or min(t.shape) < 1 or tuple(t.shape) != tuple(pitch.shape):
            raise ValueError(' - ERROR, f0_viterbi_batch: {} must be [B, F, n_cand], the same for pitch, cost and f0'.format(name))
        if torch.is_tensor(t) and t.dtype != torch.float32:
            raise ValueError(' - ERROR, f0_viterbi_batch: {} must be float32, got {}'.format(name, t.dtype))
    B, F, n_cand = (int(v) for v in pitch.shape)
    if getattr(n, 'ndim', 0) != 2 or tuple(n.shape) != (B, F):
        raise ValueError(' - ERROR, f0_viterbi_batch: n must be [B, F] = {}'.format((B, F)))
    if (n.dtype != torch.int32) if torch.is_tensor(n) else (np.asarray(n).dtype.kind not in 'iu'):
        raise ValueError(' - ERROR, f0_viterbi_batch: n must be an int32 tensor or an integer array, got {}'.format(n.dtype))
    _track_args(n_cand, 1.0, 'f0_viterbi_batch')
    costs = _viterbi_costs(unvoiced_cost, jump_cost, switch_cost, 'f0_viterbi_batch')
    h = _check_lens(lens, B, F, 'f0_viterbi_batch: lens')
    if B > 65535 or F > F0_MAX_SAMPLES + 1:
        raise ValueError(' - ERROR, f0_viterbi_batch: at most 65535 utterances of at most {} frames'.format(F0_MAX_SAMPLES + 1))
    _need_gpu('f0_viterbi_batch')
    d_frames, = _upload_lens(h)
    if not torch.is_tensor(n):
        n = torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32))
    n = n.to('cuda').contiguous()
    out = _f0_viterbi_launch(_to_device(pitch, torch.float32), _to_device(cost, torch.float32), n, d_frames, costs,
                             None if f0 is None else _to_device(f0, torch.float32))
    return _F0_PATH(*out)


def f0_track_batch(wav, lens=None, sr=16000, hop_length=80, frame_length=512, fmin=60.0, fmax=400.0, threshold=0.15, jump_cost=0.5,
                   switch_cost=0.1, n_cand=8, ceiling=1.0):
    """F0 of B utterances by Viterbi decoding over YIN's candidates: f0_candidates_batch, then f0_viterbi_batch with
    unvoiced_cost = threshold.  Where f0_batch takes the first dip of d' below the threshold, frame by frame (and reports
    the octave above when the dip at half the period slips under it), this takes the path of least cost through up to
    n_cand dips per frame.  With jump_cost = switch_cost = 0 its voicing is f0_batch's on every frame.

    Arguments as f0_batch, plus the path's costs.  Returns a namedtuple with f0_batch's fields in f0_batch's shapes and
    dtypes -- f0 [B, Fmax] (0 = unvoiced), aperiodicity [B, Fmax] (bit-identical to f0_batch's), n_frames -- so it goes
    wherever f0_batch's result goes, plus state int32 [B, Fmax] and total float32 [B] as in f0_viterbi_batch.  The
    defaults 0.5 and 0.1 come from synthetic signals with a weak fundamental, not from speech."""
    import torch
    B, Lmax = _check_wav(wav, 'f0_track_batch')
    args = _f0_args(sr, hop_length, frame_length, fmin, fmax, threshold, 'f0_track_batch')
    n_cand, ceiling = _track_args(n_cand, ceiling, 'f0_track_batch')
    costs = _viterbi_costs(args[5], jump_cost, switch_cost, 'f0_track_batch')
    h = np.full((B,), Lmax, dtype=np.int64) if lens is None else _check_lens(lens, B, Lmax, 'f0_track_batch: lens')
    _need_gpu('f0_track_batch')
    frames = [1 + int(v) // args[1] for v in h]
    d_len, d_frames = _upload_lens(h, frames)
    f0, ap, state, total = _f0_track_launch(_to_device(wav, torch.float32), d_len, d_frames, args, n_cand, ceiling, costs)
    return _F0_TRACK(f0, ap, frames, state, total)


def _check_track(t, what):
    import torch
    if getattr(t, 'ndim', 0) != 2 or min(t.shape) < 1:
        raise ValueError(' - ERROR, f0_metrics_batch: {} must be [B, F]'.format(what))
    if torch.is_tensor(t) and t.dtype != torch.float32:
        raise ValueError(' - ERROR, f0_metrics_batch: {} must be float32, got {}'.format(what, t.dtype))
    return int(t.shape[0]), int(t.shape[1])


def f0_metrics_batch(f0_a, f0_b, len_a, len_b, path=None, path_len=None):
    """F0 and voicing error of B pairs of tracks (vc_f0_metrics_f32): f0_a [B, Fa_max], f0_b [B, Fb_max] float32, 0 =
    unvoiced, as f0_batch returns them; len_a, len_b host integers.

    path, path_len: what mcd_batch(..., return_path=True) returns (int32 [B, P, 2] and int32 [B], on the device), so
    both figures are taken along one DTW path; None: the cells (i, i), i < min(len_a, len_b).
    Returns a namedtuple of [B] device tensors: n_cells, n_both_voiced, n_vuv_mismatch (int32), vuv_error =
    n_vuv_mismatch / n_cells, f0_rmse_cents = sqrt(mean (1200 log2(fa / fb))^2) and f0_rmse_hz over the both-voiced cells,
    logf0_corr = Pearson correlation of log2 f0 over them.  NaN where undefined: the RMSE values without a both-voiced
    cell, the correlation with fewer than two or when one side's f0 is the same in all of them."""
    import torch
    B, Fa = _check_track(f0_a, 'f0_a')
    Bb, Fb = _check_track(f0_b, 'f0_b')
    if B != Bb:
        raise ValueError(' - ERROR, f0_metrics_batch: f0_a {} and f0_b {} must agree in B'.format(tuple(f0_a.shape), tuple(f0_b.shape)))
    h_la, h_lb = _check_lens(len_a, B, Fa, 'f0_metrics_batch: len_a'), _check_lens(len_b, B, Fb, 'f0_metrics_batch: len_b')
    if (path is None) != (path_len is None):
        raise ValueError(' - ERROR, f0_metrics_batch: pass path and path_len together (both from mcd_batch(return_path=True)) or neither')
    if path is not None:
        if not (torch.is_tensor(path) and torch.is_tensor(path_len)) or path.dtype != torch.int32 or path_len.dtype != torch.int32:
            raise ValueError(' - ERROR, f0_metrics_batch: path and path_len must be int32 tensors')
        if path.ndim != 3 or path.shape[0] != B or path.shape[1] < 1 or path.shape[2] != 2 or tuple(path_len.shape) != (B,):
            raise ValueError(' - ERROR, f0_metrics_batch: path must be [B, P, 2] and path_len [B] (got {} and {})'
                             .format(tuple(path.shape), tuple(path_len.shape)))
    if B > 65535 or max(Fa, Fb, 0 if path is None else int(path.shape[1])) > F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, f0_metrics_batch: at most 65535 pairs of at most {} frames or cells'.format(F0_MAX_SAMPLES))
    _need_gpu('f0_metrics_batch')
    d_la, d_lb = _upload_lens(h_la, h_lb)
    if path is not None:
        path, path_len = path.to('cuda').contiguous(), path_len.to('cuda').contiguous()
    return _f0_metrics_launch(_to_device(f0_a, torch.float32), _to_device(f0_b, torch.float32), d_la, d_lb, path, path_len)


def score_wav_batch(wav_a, lens_a, wav_b, lens_b, cfg_d, wav_sr_a=None, wav_sr_b=None, res_type='kaiser_best', scale=None,
                    n_coef=24, align='dtw', band=None, first_coef=1, frame_length=512, fmin=60.0, fmax=400.0, threshold=0.15,
                    mask=None, top_db=40.0, max_gap=20, min_run=0, f0_method='yin', jump_cost=0.5, switch_cost=0.1, n_cand=8):
    """The three figures of a pair of utterances in one call -- MCD, F0 error, voiced / unvoiced error -- along ONE path.

    Arguments as mcd_wav_batch (the path is always made with align='dtw'), plus the tracker's frame_length, fmin, fmax,
    threshold.  F0 is taken from each side's waveform at cfg_d['sample_rate'] (after the resampler) with hop_length =
    cfg_d['hop_length'], so its frames are the mel frames the path indexes.  Returns a namedtuple of device tensors:
    mcd, total, path_len, path exactly as mcd_wav_batch(..., return_path=True) gives them (total, path_len, path are None
    with align='frame'), the seven fields of f0_metrics_batch, f0_a [B, Fa_max], f0_b [B, Fb_max], and n_active_a,
    n_active_b, mask_a, mask_b (None without a mask).

    mask, top_db, max_gap, min_run as in mcd_wav_batch; the voiced modes reuse the tracks computed anyway.  With a mask
    mcd, total and path_len come from the DTW over the kept frames, path is in original frame numbers and the F0 figures
    are taken along it on the original tracks (align='frame': over the frames set in both masks).  n_active == 0 marks
    a side that kept all its frames because none was active.

    f0_method='viterbi' takes both tracks from f0_track_batch's launches (jump_cost, switch_cost, n_cand; unvoiced_cost =
    threshold) instead of f0_batch's; everything that does not read a track (mcd, total, path_len, path without a voiced
    mask) is bit-identical either way."""
    import audio_lib
    if cfg_d is None:
        raise ValueError(' - ERROR, score_wav_batch: cfg_d (the data-set configuration) is required')
    if f0_method not in F0_METHODS:
        raise ValueError(' - ERROR, score_wav_batch: f0_method must be one of {}, got {!r}'.format(F0_METHODS, f0_method))
    audio_lib._res_params(res_type)
    a = _wav_side(wav_a, lens_a, cfg_d, wav_sr_a, 'wav_a')
    b = _wav_side(wav_b, lens_b, cfg_d, wav_sr_b, 'wav_b')
    if a['B'] != b['B']:
        raise ValueError(' - ERROR, score_wav_batch: wav_a and wav_b must hold the same number of utterances')
    n_coef, first_coef = int(n_coef), int(first_coef)
    scale, band = _mcd_args(cfg_d, scale, n_coef, first_coef, align, band, int(cfg_d['n_mels']))
    if align == 'dtw':
        _check_pairs(a['B'], a['Fmax'], b['Fmax'], n_coef, True)
    elif a['B'] > 65535:
        raise ValueError(' - ERROR, score_wav_batch: at most 65535 pairs')
    args = _f0_args(cfg_d['sample_rate'], cfg_d['hop_length'], frame_length, fmin, fmax, threshold, 'score_wav_batch')
    if f0_method == 'viterbi':
        n_cand, _ = _track_args(n_cand, 1.0, 'score_wav_batch')
        costs = _viterbi_costs(args[5], jump_cost, switch_cost, 'score_wav_batch')
        track = lambda x, d_len, d_fr: _f0_track_launch(x, d_len, d_fr, args, n_cand, 1.0, costs)[0]
    else:
        track = lambda x, d_len, d_fr: _f0_launch(x, d_len, args)[0]
    if mask is not None:
        act = _activity_args(mask, top_db, max_gap, min_run, 'score_wav_batch')
        _check_energy(cfg_d['hop_length'], cfg_d['win_length'], max(a['Fmax'], b['Fmax']), 'score_wav_batch')
    _need_gpu('score_wav_batch')
    d_in_a, d_len_a, d_fa, d_in_b, d_len_b, d_fb = _upload_lens(a['h_in'], a['h'], a['n_frames'], b['h_in'], b['h'], b['n_frames'])
    x_a = _wav_at_rate(wav_a, a, d_in_a, cfg_d, res_type)
    x_b = _wav_at_rate(wav_b, b, d_in_b, cfg_d, res_type)
    if mask is not None:
        x_a, x_b = x_a.contiguous(), x_b.contiguous()
        f0_a, f0_b = track(x_a, d_len_a, d_fa), track(x_b, d_len_b, d_fb)
        ma = _wav_mask(x_a, d_len_a, d_fa, cfg_d, act, f0_a)
        mb = _wav_mask(x_b, d_len_b, d_fb, cfg_d, act, f0_b)
        ia, ib = _compact_launch(ma, d_fa), _compact_launch(mb, d_fb)
        ca = _cepstra_launch(_speech_mel(x_a, d_len_a, ma, ia.n_active, cfg_d), n_coef, first_coef)
        cb = _cepstra_launch(_speech_mel(x_b, d_len_b, mb, ib.n_active, cfg_d), n_coef, first_coef)
        if align == 'frame':
            r, ic = _masked_frame(ca, cb, d_fa, d_fb, ma, mb, scale)
            cells = _path_map_launch(None, ic.n_kept, ic.index, ic.index, ic.index.shape[1])
            m = _f0_metrics_launch(f0_a, f0_b, d_fa, d_fb, cells, ic.n_kept)
            return _SCORE(r.mcd, None, None, None, *m, f0_a, f0_b, ic.n_active, ic.n_active, ma, mb)
        r = _masked_dtw(ca, cb, ia, ib, scale, band, True)
        m = _f0_metrics_launch(f0_a, f0_b, d_fa, d_fb, r.path, r.path_len)
        return _SCORE(r.mcd, r.total, r.path_len, r.path, *m, f0_a, f0_b, ia.n_active, ib.n_active, ma, mb)
    ca = _cepstra_launch(_mel_launch(x_a, d_len_a, cfg_d), n_coef, first_coef)
    cb = _cepstra_launch(_mel_launch(x_b, d_len_b, cfg_d), n_coef, first_coef)
    f0_a, f0_b = track(x_a.contiguous(), d_len_a, d_fa), track(x_b.contiguous(), d_len_b, d_fb)
    r = _frame_launch(ca, cb, d_fa, d_fb, scale) if align == 'frame' else _dtw_launch(ca, cb, d_fa, d_fb, scale, band, True)
    m = _f0_metrics_launch(f0_a, f0_b, d_fa, d_fb, r.path, r.path_len if r.path is not None else None)
    return _SCORE(r.mcd, r.total, r.path_len, r.path, *m, f0_a, f0_b, None, None, None, None)


# ------------------------------------------------------------------------------------- speech activity (csrc/vc_activity.hip)
def _activity_args(mode, top_db, max_gap, min_run, what):
    """Host checks of the mask's parameters; returns (mode bits, ratio as a float32 value, max_gap, min_run)."""
    if mode not in _MODES:
        raise ValueError(" - ERROR, {}: mode must be 'energy', 'voiced' or 'energy+voiced', got {!r}".format(what, mode))
    for v, name in ((max_gap, 'max_gap'), (min_run, 'min_run')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v >= 2 ** 31:
            raise ValueError(' - ERROR, {}: {} must be a non-negative integer number of frames, got {!r}'.format(what, name, v))
    try:
        db = float(top_db)
    except (TypeError, ValueError):
        db = float('nan')
    ratio = np.float32(10.0 ** (-db / 10.0)) if np.isfinite(db) and db > 0.0 else np.float32(0.0)
    if not (0.0 < float(ratio) < 1.0):
        raise ValueError(' - ERROR, {}: top_db must be finite and positive, with 10^(-top_db / 10) a float32 inside (0, 1); got {!r}'
                         .format(what, top_db))
    return _MODES[mode], float(ratio), int(max_gap), int(min_run)


def _check_energy(hop_length, frame_length, Fmax, what):
    for v, name, top in ((hop_length, 'hop_length', F0_MAX_HOP), (frame_length, 'frame_length', ACT_MAX_W)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v > top:
            raise ValueError(' - ERROR, {}: {} must be an integer in [1, {}], got {!r}'.format(what, name, top, v))
    if Fmax > MAX_FRAMES:
        raise ValueError(' - ERROR, {}: a mask holds at most {} frames per utterance (got {})'.format(what, MAX_FRAMES, Fmax))


def _check_mask(mask, B, F, what):
    import torch
    if F > MAX_FRAMES:
        raise ValueError(' - ERROR, {}: a mask holds at most {} frames per utterance (got {})'.format(what, MAX_FRAMES, F))
    if mask is None:
        return
    ok = (torch.uint8, torch.bool) if torch.is_tensor(mask) else (np.dtype(np.uint8), np.dtype(np.bool_))
    if getattr(mask, 'ndim', 0) != 2 or getattr(mask, 'dtype', None) not in ok:
        raise ValueError(' - ERROR, {} must be a uint8 or bool array [B, F], got {} {}'.format(what, getattr(mask, 'dtype', type(mask)),
                                                                                              tuple(getattr(mask, 'shape', ()))))
    if tuple(int(v) for v in mask.shape) != (B, F):
        raise ValueError(' - ERROR, {} must be [{}, {}] like its spectrogram, got {}'.format(what, B, F, tuple(mask.shape)))


def _mask_to_device(mask, B, F):
    import torch
    if mask is None:
        return torch.ones((B, F), dtype=torch.uint8, device='cuda')
    if not torch.is_tensor(mask):
        mask = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8))
    return mask.to(device='cuda', dtype=torch.uint8).contiguous()


def _energy_launch(wav, d_len, hop, W):
    """wav: cuda, contiguous float32 [B, Lmax]; d_len: device int32 [B] or None.  No host check in here."""
    import torch
    B, Lmax = wav.shape
    Fmax = 1 + Lmax // hop
    e = torch.empty((B, Fmax), dtype=torch.float32, device=wav.device)
    _vc.check(_vc.lib().vc_frame_energy_f32(_vc.ptr(wav), _vc.ptr(d_len), B, Lmax, Lmax, hop, W, _vc.ptr(e), Fmax, _vc.current_stream()))
    return e


def _mask_launch(energy, f0, d_frames, act):
    import torch
    mode, ratio, max_gap, min_run = act
    B, Fmax = energy.shape
    mask = torch.empty((B, Fmax), dtype=torch.uint8, device=energy.device)
    _vc.check(_vc.lib().vc_activity_mask(_vc.ptr(energy), _vc.ptr(f0) if mode & 2 else None, _vc.ptr(d_frames), B, Fmax, mode, ratio,
                                         max_gap, min_run, _vc.ptr(mask), _vc.current_stream()))
    return mask


def _compact_launch(mask_a, d_fa, mask_b=None, d_fb=None):
    import torch
    B, Fa = mask_a.shape
    dev = mask_a.device
    index = torch.empty((B, Fa), dtype=torch.int32, device=dev)
    counts = torch.empty((3, B), dtype=torch.int32, device=dev)
    intervals = torch.empty((B, (Fa + 1) // 2, 2), dtype=torch.int32, device=dev)
    _vc.check(_vc.lib().vc_mask_compact(_vc.ptr(mask_a), _vc.ptr(d_fa), Fa, _vc.ptr(mask_b), _vc.ptr(d_fb),
                                        0 if mask_b is None else mask_b.shape[1], B, _vc.ptr(index), _vc.ptr(counts[0]), _vc.ptr(counts[1]),
                                        _vc.ptr(intervals), _vc.ptr(counts[2]), _vc.current_stream()))
    return _COMPACT(index, counts[0], counts[1], intervals, counts[2])


def _rows_launch(x, index, n_kept):
    import torch
    B, F, C = x.shape
    out = torch.empty((B, F, C), dtype=torch.float32, device=x.device)
    _vc.check(_vc.lib().vc_compact_rows_f32(_vc.ptr(x), F, _vc.ptr(index), index.shape[1], _vc.ptr(n_kept), B, C, _vc.ptr(out), F,
                                            _vc.current_stream()))
    return out


def _path_map_launch(path, path_len, index_a, index_b, max_path):
    """path None: the cells (p, p), p < path_len."""
    import torch
    B = index_a.shape[0]
    out = torch.empty((B, max_path, 2), dtype=torch.int32, device=index_a.device)
    _vc.check(_vc.lib().vc_path_map(_vc.ptr(path), _vc.ptr(path_len), B, max_path, _vc.ptr(index_a), index_a.shape[1], _vc.ptr(index_b),
                                    index_b.shape[1], _vc.ptr(out), _vc.current_stream()))
    return out


def _wav_mask(x, d_len, d_frames, cfg_d, act, f0):
    """The mask of one side of the cfg_d-level calls: x at cfg_d['sample_rate'], the energy over win_length samples."""
    return _mask_launch(_energy_launch(x, d_len, int(cfg_d['hop_length']), int(cfg_d['win_length'])), f0, d_frames, act)


def _speech_mel(x, d_len, mask, n_active, cfg_d):
    """The front-end's mel of x with the amplitude normalisation taken over the samples of the active frames
    (vc_speech_gain_f32, include/vc_hip.h): the same speech gives the same mel whatever silence surrounds it.  With
    cfg_d['mean_abs_amp_norm'] == 1 the front-end does not normalise and nothing is to be done."""
    import torch
    target = float(cfg_d['mean_abs_amp_norm'])
    if target == 1.0:
        return _mel_launch(x, d_len, cfg_d)
    lib, st = _vc.lib(), _vc.current_stream()
    B, Lmax = x.shape
    gain = torch.empty((B,), dtype=torch.float32, device=x.device)
    _vc.check(lib.vc_speech_gain_f32(_vc.ptr(x), _vc.ptr(d_len), B, Lmax, Lmax, int(cfg_d['hop_length']), _vc.ptr(mask), _vc.ptr(n_active),
                                     mask.shape[1], target, _vc.ptr(gain), st))
    y = torch.empty_like(x)
    _vc.check(lib.vc_scale_rows_f32(_vc.ptr(x), _vc.ptr(d_len), B, Lmax, Lmax, _vc.ptr(gain), _vc.ptr(y), st))
    return _mel_launch(y, d_len, cfg_d, amp_norm=1.0)


def _masked_dtw(ca, cb, ia, ib, scale, band, return_path):
    """Each side compacted by its own list (ia, ib: _compact_launch), the DTW over the kept frames, the path mapped back to
    original frame numbers."""
    r = _dtw_launch(_rows_launch(ca, ia.index, ia.n_kept), _rows_launch(cb, ib.index, ib.n_kept), ia.n_kept, ib.n_kept, scale, band,
                    return_path)
    if return_path:
        r = r._replace(path=_path_map_launch(r.path, r.path_len, ia.index, ib.index, r.path.shape[1]))
    return r


def _masked_frame(ca, cb, d_fa, d_fb, ma, mb, scale):
    """One common list, the frames set in both masks, for both sides."""
    ic = _compact_launch(ma, d_fa, mb, d_fb)
    return _frame_launch(_rows_launch(ca, ic.index, ic.n_kept), _rows_launch(cb, ic.index, ic.n_kept), ic.n_kept, ic.n_kept, scale), ic


def activity_batch(wav, lens=None, hop_length=80, frame_length=400, mode='energy', top_db=40.0, max_gap=20, min_run=0, f0=None,
                   sr=16000, fmin=60.0, fmax=400.0, threshold=0.15, yin_frame_length=512):
    """Where the speech is, per frame (the definitions are in include/vc_hip.h, "Speech activity").

    wav [B, Lmax] float32 (cuda tensor or numpy array); lens: host integers in [1, Lmax] (None = the whole row).
    Frames are the front-end's and the tracker's: 1 + len // hop_length, Fmax = 1 + Lmax // hop_length <= 16384.
    mode 'energy': the frame's energy over frame_length samples is positive and above 10^(-top_db / 10) of the
    utterance's largest; 'voiced': the tracker's f0 > 0 (``f0`` [B, Fmax] as f0_batch returns it, or None: the tracker is
    run here with sr, fmin, fmax, threshold, yin_frame_length); 'energy+voiced': both.  Then gaps of at most max_gap frames
    between active frames are filled and active runs shorter than min_run dropped.
    Returns a namedtuple of device tensors: mask [B, Fmax] uint8; index [B, Fmax] int32, the active frames ascending, -1
    beyond n_kept; n_active [B]; n_kept [B] = n_active, or the frame count where n_active is 0 (index = 0 .. F-1);
    intervals [B, (Fmax + 1) // 2, 2] int32, the runs as [start, end), -1 beyond n_intervals [B]; energy [B, Fmax] float32;
    and n_frames, a host list."""
    import torch
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, activity_batch: wav must be [B, Lmax]')
    if torch.is_tensor(wav) and wav.dtype != torch.float32:
        raise ValueError(' - ERROR, activity_batch: wav must be float32, got {}'.format(wav.dtype))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    act = _activity_args(mode, top_db, max_gap, min_run, 'activity_batch')
    if isinstance(hop_length, bool) or not isinstance(hop_length, (int, np.integer)) or hop_length < 1:
        raise ValueError(' - ERROR, activity_batch: hop_length must be a positive integer, got {!r}'.format(hop_length))
    Fmax = 1 + Lmax // int(hop_length)
    _check_energy(hop_length, frame_length, Fmax, 'activity_batch')
    hop, W = int(hop_length), int(frame_length)
    h = np.full((B,), Lmax, dtype=np.int64) if lens is None else _check_lens(lens, B, Lmax, 'activity_batch: lens')
    if B > 65535 or Lmax > F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, activity_batch: at most 65535 utterances of at most {} samples (got {} of {})'.format(F0_MAX_SAMPLES, B, Lmax))
    args = None
    if act[0] & 2:
        if f0 is None:
            args = _f0_args(sr, hop, yin_frame_length, fmin, fmax, threshold, 'activity_batch')
        elif getattr(f0, 'ndim', 0) != 2 or tuple(int(v) for v in f0.shape) != (B, Fmax) or \
                (f0.dtype != torch.float32 if torch.is_tensor(f0) else np.asarray(f0).dtype != np.float32):
            raise ValueError(' - ERROR, activity_batch: f0 must be float32 [{}, {}], as f0_batch returns it'.format(B, Fmax))
    _need_gpu('activity_batch')
    n_frames = 1 + h // hop
    d_len, d_frames = _upload_lens(h, n_frames)
    x = _to_device(wav, torch.float32)
    energy = _energy_launch(x, d_len, hop, W)
    if act[0] & 2:
        f0 = _f0_launch(x, d_len, args)[0] if f0 is None else _to_device(f0, torch.float32)
    mask = _mask_launch(energy, f0, d_frames, act)
    c = _compact_launch(mask, d_frames)
    return _ACTIVITY(mask, c.index, c.n_active, c.n_kept, c.intervals, c.n_intervals, energy, [int(n) for n in n_frames])


def compact_batch(x, index, n_kept):
    """out[b, k, :] = x[b, index[b, k], :] for k < n_kept[b], zeros beyond (vc_compact_rows_f32): x [B, F, C] float32, index
    [B, Fi] int32 and n_kept [B] int32 as activity_batch returns them (device tensors).  Returns [B, F, C] on the device."""
    import torch
    if getattr(x, 'ndim', 0) != 3 or min(x.shape) < 1:
        raise ValueError(' - ERROR, compact_batch: x must be [B, F, C]')
    if torch.is_tensor(x) and x.dtype != torch.float32:
        raise ValueError(' - ERROR, compact_batch: x must be float32, got {}'.format(x.dtype))
    B, F, C = (int(v) for v in x.shape)
    if not (torch.is_tensor(index) and torch.is_tensor(n_kept)) or index.dtype != torch.int32 or n_kept.dtype != torch.int32:
        raise ValueError(' - ERROR, compact_batch: index and n_kept must be int32 tensors')
    if index.ndim != 2 or index.shape[0] != B or index.shape[1] < 1 or tuple(n_kept.shape) != (B,):
        raise ValueError(' - ERROR, compact_batch: index must be [B, Fi] and n_kept [B] (got {} and {})'.format(tuple(index.shape), tuple(n_kept.shape)))
    if B > 65535 or F > MAX_FRAMES or index.shape[1] > MAX_FRAMES or C > ACT_MAX_COLS:
        raise ValueError(' - ERROR, compact_batch: at most 65535 utterances of at most {} frames of at most {} columns'.format(MAX_FRAMES, ACT_MAX_COLS))
    _need_gpu('compact_batch')
    return _rows_launch(_to_device(x, torch.float32), index.to('cuda').contiguous(), n_kept.to('cuda').contiguous())


# ------------------------------------------------------------------------------------- content (csrc/vc_content.hip)
# The usual folding of TIMIT's 61 phones to 39 (Lee and Hon 1989): a name on the left is scored as the name on the right.
# The closures join the pauses in one silence class, whose representative here is 'pau'; 'q' (the glottal stop) is
# deleted (None).  A name that is not listed stands for itself.
TIMIT_FOLD_39 = {'ao': 'aa', 'ax': 'ah', 'ax-h': 'ah', 'axr': 'er', 'hv': 'hh', 'ix': 'ih', 'el': 'l', 'em': 'm', 'en': 'n', 'nx': 'n',
                 'eng': 'ng', 'zh': 'sh', 'ux': 'uw', 'pcl': 'pau', 'tcl': 'pau', 'kcl': 'pau', 'bcl': 'pau', 'dcl': 'pau', 'gcl': 'pau',
                 'epi': 'pau', 'h#': 'pau', 'q': None}


def class_map(names, fold=TIMIT_FOLD_39, drop=('pau', 'epi', 'h#')):
    """The int32 table [C] the content calls take as ``class_map``, for a phoneme inventory ``names``
    (sound_ds.TIMIT_PHONEMES_61, sound_ds.ARCTIC_PHONEMES_43): table[c] is the index IN ``names`` of the representative of
    class c under ``fold`` (None or {}: every class stands for itself), so the table stays [C]; -1 for a class the fold
    deletes and for every class NAMED in ``drop``.  A class that folds onto a dropped representative keeps that
    representative's index: with the defaults the six closures of TIMIT score as one silence symbol (the index of 'pau')
    while the pauses themselves ('pau', 'epi', 'h#') leave the sequence -- 39 distinct labels stay.  Names of ``fold`` and
    ``drop`` that the inventory lacks are ignored; a representative the inventory lacks leaves the class to itself."""
    names = list(names)
    if not names or len(set(names)) != len(names) or not all(isinstance(n, str) for n in names):
        raise ValueError(' - ERROR, class_map: names must be a non-empty list of distinct strings')
    if len(names) > CONTENT_MAX_CLASSES:
        raise ValueError(' - ERROR, class_map: at most {} classes (got {})'.format(CONTENT_MAX_CLASSES, len(names)))
    pos = {n: i for i, n in enumerate(names)}
    table = np.arange(len(names), dtype=np.int32)
    for n, rep in (fold or {}).items():
        if n in pos:
            table[pos[n]] = -1 if rep is None else pos.get(rep, pos[n])
    for n in drop or ():
        if n in pos:
            table[pos[n]] = -1
    return table


CONTENT_MAX_CLASSES = 256   # vc_ppg_metrics_f32, vc_phn_segments
SEGMENT_TILE = 1024         # vc_phn_segments_tile(): frames per tile of the segment kernel
EDIT_ROWS = 256             # vc_edit_distance_rows(): symbols of A per pass of the edit-distance kernel
EDIT_MAX = 16384            # vc_edit_distance_i32
_PPG_FIELDS = 'n_cells n_agree frame_agreement js_mean'
_EDIT_FIELDS = 'dist n_match n_sub n_del n_ins per'
_PPG = namedtuple('ppg_metrics', _PPG_FIELDS)
_SEG = namedtuple('phn_segments', 'labels start end n_seg')
_EDIT = namedtuple('edit_distance', _EDIT_FIELDS)
_CONTENT = namedtuple('content', _PPG_FIELDS + ' ' + _EDIT_FIELDS + ' seg_a seg_b')
_CONTENT_WAV = namedtuple('content_wav', _PPG_FIELDS + ' ' + _EDIT_FIELDS + ' seg_a seg_b ppg_a ppg_b len_a len_b path path_len mask_a mask_b')


def _check_ppg(x, what):
    import torch
    if getattr(x, 'ndim', 0) != 3 or min(x.shape) < 1:
        raise ValueError(' - ERROR, {} must be [B, F, C]'.format(what))
    dt = x.dtype if torch.is_tensor(x) else np.asarray(x).dtype
    if dt not in (torch.float32, np.dtype(np.float32)):
        raise ValueError(' - ERROR, {} must be float32, got {}'.format(what, dt))
    B, F, C = (int(v) for v in x.shape)
    if C > CONTENT_MAX_CLASSES:
        raise ValueError(' - ERROR, {}: at most {} classes (got {})'.format(what, CONTENT_MAX_CLASSES, C))
    if B > 65535 or F > F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, {}: at most 65535 rows of at most {} frames (got {} of {})'.format(what, F0_MAX_SAMPLES, B, F))
    return B, F, C


def _check_class_map(cmap, C, what, allow_drop=True):
    """None, or C integers in [-1, C) (a device tensor is taken as it is: int32 [C], its values unread)."""
    import torch
    if cmap is None:
        return None
    if torch.is_tensor(cmap) and cmap.is_cuda:
        if cmap.dtype != torch.int32 or tuple(cmap.shape) != (C,):
            raise ValueError(' - ERROR, {}: a class_map on the device must be int32 [{}]'.format(what, C))
        return cmap
    h = np.asarray(cmap.cpu() if torch.is_tensor(cmap) else cmap)
    if h.shape != (C,) or h.dtype.kind not in 'iu' or h.min() < -1 or h.max() >= C:
        raise ValueError(' - ERROR, {}: class_map must be {} integers in [-1, {}) (evaluation.class_map builds one)'.format(what, C, C))
    return h.astype(np.int32)


def _check_min_run(min_run, what):
    if isinstance(min_run, bool) or not isinstance(min_run, (int, np.integer)) or min_run < 1 or min_run >= 2 ** 31:
        raise ValueError(' - ERROR, {}: min_run must be a positive integer number of frames, got {!r}'.format(what, min_run))
    return int(min_run)


def _check_counts(n, B, lo, hi, what):
    """Host integers in [lo, hi], or an int32 [B] tensor on the device (the launch clamps it).  Returns (host array | None,
    device tensor | None)."""
    import torch
    if torch.is_tensor(n) and n.is_cuda:
        if n.dtype != torch.int32 or tuple(n.shape) != (B,):
            raise ValueError(' - ERROR, {} on the device must be int32 [{}]'.format(what, B))
        return None, n.contiguous()
    h = np.asarray(n.cpu() if torch.is_tensor(n) else n)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < lo or h.max() > hi:
        raise ValueError(' - ERROR, {} must be {} integers in [{}, {}]'.format(what, B, lo, hi))
    return h.astype(np.int64), None


def _check_path(path, path_len, B, what):
    import torch
    if (path is None) != (path_len is None):
        raise ValueError(' - ERROR, {}: pass path and path_len together (both from mcd_batch(return_path=True)) or neither'.format(what))
    if path is None:
        return
    if not (torch.is_tensor(path) and torch.is_tensor(path_len)) or path.dtype != torch.int32 or path_len.dtype != torch.int32:
        raise ValueError(' - ERROR, {}: path and path_len must be int32 tensors'.format(what))
    if path.ndim != 3 or path.shape[0] != B or path.shape[1] < 1 or path.shape[2] != 2 or tuple(path_len.shape) != (B,):
        raise ValueError(' - ERROR, {}: path must be [B, P, 2] and path_len [B] (got {} and {})'.format(what, tuple(path.shape), tuple(path_len.shape)))
    if path.shape[1] > F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, {}: at most {} cells'.format(what, F0_MAX_SAMPLES))


def _upload_mixed(*items):
    """items: (host array | None, device tensor | None) pairs; the host ones go up in one pinned copy."""
    hosts = [h for h, d in items if d is None]
    ups = iter(_upload_lens(*hosts)) if hosts else iter(())
    return [next(ups) if d is None else d for h, d in items]


def _cmap_device(cmap):
    import torch
    if cmap is None or torch.is_tensor(cmap):
        return cmap
    return torch.from_numpy(cmap).pin_memory().to('cuda', non_blocking=True)


def _ppg_metrics_launch(a, b, d_la, d_lb, path, path_len, cmap):
    """a, b: cuda, contiguous float32 [B, F, C]; lengths, path, map on the device.  No host check in here."""
    import torch
    B, Fa, C = a.shape
    counts = torch.empty((B, 2), dtype=torch.int32, device=a.device)
    values = torch.empty((B, 2), dtype=torch.float32, device=a.device)
    _vc.check(_vc.lib().vc_ppg_metrics_f32(_vc.ptr(a), _vc.ptr(b), _vc.ptr(d_la), _vc.ptr(d_lb), B, Fa, b.shape[1], C, _vc.ptr(path),
                                           _vc.ptr(path_len), 0 if path is None else path.shape[1], _vc.ptr(cmap), _vc.ptr(counts),
                                           _vc.ptr(values), _vc.current_stream()))
    return _PPG(counts[:, 0], counts[:, 1], values[:, 0], values[:, 1])


def _segments_launch(ppg, d_len, cmap, min_run):
    import torch
    B, F, C = ppg.shape
    out = torch.empty((3, B, F), dtype=torch.int32, device=ppg.device)
    n_seg = torch.empty((B,), dtype=torch.int32, device=ppg.device)
    _vc.check(_vc.lib().vc_phn_segments(_vc.ptr(ppg), _vc.ptr(d_len), B, F, C, min_run, _vc.ptr(cmap), _vc.ptr(out[0]), _vc.ptr(out[1]),
                                        _vc.ptr(out[2]), _vc.ptr(n_seg), _vc.current_stream()))
    return _SEG(out[0], out[1], out[2], n_seg)


def _edit_launch(seq_a, seq_b, d_na, d_nb):
    import torch
    lib = _vc.lib()
    B, Ma = seq_a.shape
    Mb = seq_b.shape[1]
    counts = torch.empty((B, 5), dtype=torch.int32, device=seq_a.device)
    per = torch.empty((B,), dtype=torch.float32, device=seq_a.device)
    need = lib.vc_edit_distance_workspace_bytes(B, Ma, Mb)
    if need == 0:
        raise _vc.VCError('vc_edit_distance_workspace_bytes refused {} pairs of {} x {} symbols'.format(B, Ma, Mb))
    ws = torch.empty((need,), dtype=torch.uint8, device=seq_a.device)
    _vc.check(lib.vc_edit_distance_i32(_vc.ptr(seq_a), _vc.ptr(seq_b), _vc.ptr(d_na), _vc.ptr(d_nb), B, Ma, Mb, _vc.ptr(counts),
                                       _vc.ptr(per), _vc.ptr(ws), need, _vc.current_stream()))
    return _EDIT(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3], counts[:, 4], per)


def ppg_metrics_batch(ppg_a, ppg_b, len_a, len_b, path=None, path_len=None, class_map=None):
    """Frame-level agreement of B pairs of phoneme posteriorgrams (vc_ppg_metrics_f32): ppg_a [B, Fa_max, C], ppg_b
    [B, Fb_max, C] float32 (cuda tensor or numpy array), C <= 256; len_a, len_b host integers in [1, F_max].
    path, path_len: as in f0_metrics_batch (what mcd_batch(..., return_path=True) returns); None: the cells (i, i).
    class_map: None or C integers (evaluation.class_map), applied to the arg-max before the comparison.
    Returns a namedtuple of [B] device tensors: n_cells, n_agree (int32), frame_agreement = n_agree / n_cells and js_mean,
    the mean Jensen-Shannon divergence of the two posteriors over the cells in bits (0 = identical, 1 = disjoint); both NaN
    without a cell."""
    import torch
    B, Fa, C = _check_ppg(ppg_a, 'ppg_metrics_batch: ppg_a')
    Bb, Fb, Cb = _check_ppg(ppg_b, 'ppg_metrics_batch: ppg_b')
    if B != Bb or C != Cb:
        raise ValueError(' - ERROR, ppg_metrics_batch: ppg_a {} and ppg_b {} must agree in B and C'.format(tuple(ppg_a.shape), tuple(ppg_b.shape)))
    h_la, h_lb = _check_lens(len_a, B, Fa, 'ppg_metrics_batch: len_a'), _check_lens(len_b, B, Fb, 'ppg_metrics_batch: len_b')
    _check_path(path, path_len, B, 'ppg_metrics_batch')
    cmap = _check_class_map(class_map, C, 'ppg_metrics_batch')
    _need_gpu('ppg_metrics_batch')
    d_la, d_lb = _upload_lens(h_la, h_lb)
    if path is not None:
        path, path_len = path.to('cuda').contiguous(), path_len.to('cuda').contiguous()
    return _ppg_metrics_launch(_to_device(ppg_a, torch.float32), _to_device(ppg_b, torch.float32), d_la, d_lb, path, path_len,
                               _cmap_device(cmap))


def phn_segments_batch(ppg, lens, class_map=None, min_run=3):
    """The phoneme sequence of B posteriorgrams (vc_phn_segments; the five steps are in include/vc_hip.h, "Content"): the
    arg-max label of every frame through ``class_map``, runs shorter than ``min_run`` frames removed, equal neighbours
    merged, segments labelled -1 removed.  ppg [B, F_max, C] float32; lens: host integers in [0, F_max] or an int32 [B]
    device tensor.  Returns a namedtuple of int32 device tensors: labels, start, end [B, F_max] (end exclusive, -1 from the
    row's count on) and n_seg [B]."""
    import torch
    B, F, C = _check_ppg(ppg, 'phn_segments_batch: ppg')
    n = _check_counts(lens, B, 0, F, 'phn_segments_batch: lens')
    cmap = _check_class_map(class_map, C, 'phn_segments_batch')
    min_run = _check_min_run(min_run, 'phn_segments_batch')
    _need_gpu('phn_segments_batch')
    d_len, = _upload_mixed(n)
    return _segments_launch(_to_device(ppg, torch.float32), d_len, _cmap_device(cmap), min_run)


def _check_seq(s, what):
    import torch
    if getattr(s, 'ndim', 0) != 2 or min(s.shape) < 1:
        raise ValueError(' - ERROR, edit_distance_batch: {} must be [B, M]'.format(what))
    dt = s.dtype if torch.is_tensor(s) else np.asarray(s).dtype
    if dt not in (torch.int32, np.dtype(np.int32)):
        raise ValueError(' - ERROR, edit_distance_batch: {} must be int32, got {}'.format(what, dt))
    return int(s.shape[0]), int(s.shape[1])


def edit_distance_batch(seq_a, seq_b, n_a, n_b):
    """Levenshtein distance of B pairs of int32 sequences with the counts behind it (vc_edit_distance_i32): seq_a [B, Ma],
    seq_b [B, Mb] (cuda tensor or numpy array, at most 16,384 columns); n_a, n_b: host integers in [0, M] or int32 [B]
    device tensors, as phn_segments_batch returns them.  A is the reference: n_del counts symbols of A without a partner,
    n_ins symbols of B without one.  Returns a namedtuple of [B] device tensors: dist, n_match, n_sub, n_del, n_ins (int32;
    dist = n_sub + n_del + n_ins, n_match + n_sub + n_del = n_a) and per = dist / n_a (float32, NaN when n_a = 0)."""
    import torch
    B, Ma = _check_seq(seq_a, 'seq_a')
    Bb, Mb = _check_seq(seq_b, 'seq_b')
    if B != Bb:
        raise ValueError(' - ERROR, edit_distance_batch: seq_a {} and seq_b {} must agree in B'.format(tuple(seq_a.shape), tuple(seq_b.shape)))
    if B > 65535 or Ma > EDIT_MAX or Mb > EDIT_MAX:
        raise ValueError(' - ERROR, edit_distance_batch: at most 65535 pairs of at most {} symbols (got {} pairs of {} x {})'
                         .format(EDIT_MAX, B, Ma, Mb))
    na, nb = _check_counts(n_a, B, 0, Ma, 'edit_distance_batch: n_a'), _check_counts(n_b, B, 0, Mb, 'edit_distance_batch: n_b')
    _need_gpu('edit_distance_batch')
    d_na, d_nb = _upload_mixed(na, nb)
    dev = lambda s: (s if torch.is_tensor(s) else torch.from_numpy(np.ascontiguousarray(s))).to('cuda').contiguous()
    return _edit_launch(dev(seq_a), dev(seq_b), d_na, d_nb)


def _content_launch(a, b, d_la, d_lb, path, path_len, cmap, min_run, ma, mb, dec=None):
    """content_batch after its checks: everything on the device.  ma, mb: uint8 masks (both or neither).  dec: None (the
    sequences are vc_phn_segments' arg-max read-outs) or _decode_args' result (they come from vc_decode_f32)."""
    seg = (lambda x, n: _segments_launch(x, n, cmap, min_run)) if dec is None else (lambda x, n: _decode_launch(x, n, cmap, dec).seg)
    if ma is None:
        m = _ppg_metrics_launch(a, b, d_la, d_lb, path, path_len, cmap)
        sa, sb = seg(a, d_la), seg(b, d_lb)
    else:
        ia, ib = _compact_launch(ma, d_la), _compact_launch(mb, d_lb)
        sa = seg(_rows_launch(a, ia.index, ia.n_kept), ia.n_kept)
        sb = seg(_rows_launch(b, ib.index, ib.n_kept), ib.n_kept)
        if path is None:                                            # the frames set in both masks, in original frame numbers
            ic = _compact_launch(ma, d_la, mb, d_lb)
            path, path_len = _path_map_launch(None, ic.n_kept, ic.index, ic.index, ic.index.shape[1]), ic.n_kept
        m = _ppg_metrics_launch(a, b, d_la, d_lb, path, path_len, cmap)
    if a.shape[1] > EDIT_MAX or b.shape[1] > EDIT_MAX:
        raise ValueError(' - ERROR, content_batch: the edit distance holds at most {} symbols a side'.format(EDIT_MAX))
    e = _edit_launch(sa.labels, sb.labels, sa.n_seg, sb.n_seg)
    return _CONTENT(*m, *e, sa, sb)


def content_batch(ppg_a, ppg_b, len_a, len_b, path=None, path_len=None, class_map=None, min_run=3, mask_a=None, mask_b=None,
                  sequence='argmax', decode=None):
    """Does the conversion still say the same thing?  The three content figures of B pairs of posteriorgrams in one call:
    ppg_metrics_batch along the cells, phn_segments_batch of both sides, and edit_distance_batch of the two phoneme
    sequences with A as the reference (per = phoneme error rate).  Arguments as in those calls; F_max <= 16,384.

    mask_a [B, Fa_max], mask_b [B, Fb_max]: uint8 or bool, 1 = the frame counts (activity_batch's mask; one of them None:
    every frame of that side).  The masked frames leave each posteriorgram (compact_batch) before its sequence is read
    off, exactly as mcd_batch compacts the cepstra; start and end of the segments then count kept frames.  The frame-level
    figures run on the original posteriorgrams along ``path``, which is in original frame numbers (what the masked
    mcd_batch(return_path=True) returns visits kept frames only), or, without a path, over the frames set in both masks.
    sequence: 'argmax' (phn_segments_batch with ``min_run``: the launches this call has always issued) or 'viterbi': the
    two sequences come from the phone-loop decoder instead (decode_batch; ``decode`` is a dict of its keyword arguments
    trans, penalty, init, final, min_dur, kind, floor; C <= 128), after the same mask compaction; ``min_run`` is unused then.
    Returns a namedtuple of device tensors: the four fields of ppg_metrics_batch, the six of edit_distance_batch, and
    seg_a, seg_b, the two results of phn_segments_batch."""
    import torch
    B, Fa, C = _check_ppg(ppg_a, 'content_batch: ppg_a')
    Bb, Fb, Cb = _check_ppg(ppg_b, 'content_batch: ppg_b')
    if B != Bb or C != Cb:
        raise ValueError(' - ERROR, content_batch: ppg_a {} and ppg_b {} must agree in B and C'.format(tuple(ppg_a.shape), tuple(ppg_b.shape)))
    if Fa > EDIT_MAX or Fb > EDIT_MAX:
        raise ValueError(' - ERROR, content_batch: at most {} frames per utterance (got {} and {})'.format(EDIT_MAX, Fa, Fb))
    h_la, h_lb = _check_lens(len_a, B, Fa, 'content_batch: len_a'), _check_lens(len_b, B, Fb, 'content_batch: len_b')
    _check_path(path, path_len, B, 'content_batch')
    cmap = _check_class_map(class_map, C, 'content_batch')
    min_run = _check_min_run(min_run, 'content_batch')
    dec = _content_sequence(sequence, decode, B, max(Fa, Fb), C, 'content_batch')
    masked = mask_a is not None or mask_b is not None
    if masked:
        _check_mask(mask_a, B, Fa, 'content_batch: mask_a')
        _check_mask(mask_b, B, Fb, 'content_batch: mask_b')
    _need_gpu('content_batch')
    d_la, d_lb = _upload_lens(h_la, h_lb)
    if path is not None:
        path, path_len = path.to('cuda').contiguous(), path_len.to('cuda').contiguous()
    ma, mb = (_mask_to_device(mask_a, B, Fa), _mask_to_device(mask_b, B, Fb)) if masked else (None, None)
    return _content_launch(_to_device(ppg_a, torch.float32), _to_device(ppg_b, torch.float32), d_la, d_lb, path, path_len,
                           _cmap_device(cmap), min_run, ma, mb, _decode_upload(dec))


def _content_side(encoder, wav, side, plan, tabs, cfg_d, res_type, window_batch, ppg):
    """One side of content_wav_batch on the device: the waveform at cfg_d['sample_rate'], the front-end, the window tables
    of convert_batch, the encoder in chunks, the stitch.  Returns (x, mel cut to the windows' frames, posteriors)."""
    import torch
    import conversion
    d_in, d_len, d_clip, d_win, d_utt, d_true = tabs
    x = _wav_at_rate(wav, side, d_in, cfg_d, res_type)
    mfcc, mel, _ = _fe_launch(x, d_len, cfg_d)
    mel_cut = conversion.cut_windows(mel, d_true, d_clip, plan.Fout)
    if ppg is None:
        win = conversion.cut_windows(mfcc, d_win, d_clip, plan.T)
        ys = [encoder.forward(win[i:i + window_batch])['y_pred'] for i in range(0, win.shape[0], window_batch)]
        ppg = conversion.compound_stitch(ys[0] if len(ys) == 1 else torch.cat(ys, 0), d_utt, plan.Fout)
    return x, mel_cut, ppg


def content_wav_batch(encoder, wav_a, lens_a, wav_b, lens_b, cfg_d, wav_sr_a=None, wav_sr_b=None, res_type='kaiser_best',
                      align='frame', band=None, scale=None, n_coef=24, first_coef=1, class_map=None, min_run=3, mask=None,
                      top_db=40.0, max_gap=20, mask_min_run=0, frame_length=512, fmin=60.0, fmax=400.0, threshold=0.15,
                      ppg_a=None, t_s=0, t_e=60, two_pass=True, window_batch=64, sequence='argmax', decode=None):
    """The content figures of B pairs of WAVEFORMS: typically A is the source and B is convert_batch(...).y_wav_pred; with
    align='dtw' B may be the target speaker's own recording.  encoder: the phoneme recogniser (encoder.encoder_spec_phn;
    decoder.encoder of a decoder built with one).

    Each side goes through the resampler (wav_sr_a / wav_sr_b), audio_lib.calc_MFCC_input_batch and the window tables of
    convert_batch (conversion.convert_plan with t_s, t_e, two_pass; cut_windows; encoder.forward in chunks of window_batch
    windows; compound_stitch), which gives posteriors [B, Fout, n_phn] whose frame f is front-end frame n_s + f, as
    convert_batch's phn_pred.  ppg_a: such posteriors of side A that are already there (phn_pred), instead of running the
    encoder on A.  The frames scored are those that come from the waveform: min(n_out, min(n_src, n_e) - n_s) per
    utterance (the zero padding that fills the last window is left out).  Then content_batch.
    align='frame': the cells (i, i).  align='dtw': along the path of the mel-cepstral DTW (``band``, ``scale``, ``n_coef``,
    ``first_coef`` as in mcd_batch) between the two mel spectrograms cut to the same frames.
    mask: None, or 'energy', 'voiced', 'energy+voiced' with top_db, max_gap, mask_min_run (activity_batch's min_run) and
    the tracker's frame_length, fmin, fmax, threshold: the masks are taken from each side's waveform as in
    score_wav_batch (energy over cfg_d['win_length'] samples) and go to content_batch and to the DTW as in
    mcd_batch(mask_a, mask_b); the mel is the front-end's own (no speech-level gain).  sequence, decode: as in
    content_batch.
    Returns a namedtuple of device tensors: content_batch's fields, then ppg_a, ppg_b [B, Fout, n_phn], len_a, len_b (int32
    [B]), path, path_len (None with align='frame') and mask_a, mask_b (None without a mask)."""
    import torch
    import audio_lib
    import conversion
    if cfg_d is None:
        raise ValueError(' - ERROR, content_wav_batch: cfg_d (the data-set configuration) is required')
    audio_lib._res_params(res_type)
    a = _wav_side(wav_a, lens_a, cfg_d, wav_sr_a, 'wav_a')
    b = _wav_side(wav_b, lens_b, cfg_d, wav_sr_b, 'wav_b')
    B = a['B']
    if B != b['B']:
        raise ValueError(' - ERROR, content_wav_batch: wav_a and wav_b must hold the same number of utterances')
    n_coef, first_coef = int(n_coef), int(first_coef)
    scale, band = _mcd_args(cfg_d, scale, n_coef, first_coef, align, band, int(cfg_d['n_mels']))
    window_batch = int(window_batch)
    if window_batch <= 0:
        raise ValueError(' - ERROR, content_wav_batch: window_batch must be positive')
    min_run = _check_min_run(min_run, 'content_wav_batch')
    pa = conversion.convert_plan(a['h'], cfg_d, t_s, t_e, two_pass)
    pb = conversion.convert_plan(b['h'], cfg_d, t_s, t_e, two_pass)
    if B > 65535 or pa.Fout > MAX_FRAMES or pb.Fout > MAX_FRAMES:
        raise ValueError(' - ERROR, content_wav_batch: at most 65535 pairs of at most {} frames (got {} pairs of {} x {})'
                         .format(MAX_FRAMES, B, pa.Fout, pb.Fout))
    if align == 'dtw':
        _check_pairs(B, pa.Fout, pb.Fout, n_coef, True)
    C = int(encoder.cfg_d['n_output'])
    if ppg_a is not None:
        if _check_ppg(ppg_a, 'content_wav_batch: ppg_a') != (B, pa.Fout, C):
            raise ValueError(' - ERROR, content_wav_batch: ppg_a must be [{}, {}, {}], as convert_batch returns phn_pred for wav_a'
                             .format(B, pa.Fout, C))
    cmap = _check_class_map(class_map, C, 'content_wav_batch')
    dec = _content_sequence(sequence, decode, B, max(pa.Fout, pb.Fout), C, 'content_wav_batch')
    if mask is not None:
        act = _activity_args(mask, top_db, max_gap, mask_min_run, 'content_wav_batch')
        _check_energy(cfg_d['hop_length'], cfg_d['win_length'], max(a['Fmax'], b['Fmax']), 'content_wav_batch')
        args = _f0_args(cfg_d['sample_rate'], cfg_d['hop_length'], frame_length, fmin, fmax, threshold, 'content_wav_batch') if act[0] & 2 else None
    h_la, h_lb = (np.minimum(p.n_out, p.n_clip - p.n_s) for p in (pa, pb))
    if min(h_la.min(), h_lb.min()) < 1:
        raise ValueError(' - ERROR, content_wav_batch: every utterance needs at least one frame of its own after t_s = {} s'.format(t_s))
    _need_gpu('content_wav_batch')
    up = _upload_lens(a['h_in'], a['h'], a['n_frames'], pa.n_clip, pa.win_tab, pa.utt_tab, pa.true_tab, h_la,
                      b['h_in'], b['h'], b['n_frames'], pb.n_clip, pb.win_tab, pb.utt_tab, pb.true_tab, h_lb)
    sides = []
    for k, (wav, side, plan, ppg) in enumerate(((wav_a, a, pa, ppg_a), (wav_b, b, pb, None))):
        d_in, d_len, d_fr, d_clip, d_win, d_utt, d_true, d_l = up[8 * k:8 * k + 8]
        if ppg is not None:
            ppg = _to_device(ppg, torch.float32)
        x, mel, ppg = _content_side(encoder, wav, side, plan, (d_in, d_len, d_clip, d_win.view(-1, 2), d_utt.view(-1, 3), d_true.view(-1, 2)),
                                    cfg_d, res_type, window_batch, ppg)
        m = None
        if mask is not None:                                        # front-end frame n_s + f is the posteriors' frame f
            x = x.contiguous()
            full = _wav_mask(x, d_len, d_fr, cfg_d, act, _f0_launch(x, d_len, args)[0] if args else None)
            n_s = int(plan.n_s[0])
            m = torch.zeros((B, plan.Fout), dtype=torch.uint8, device=full.device)
            n = max(0, min(plan.Fout, full.shape[1] - n_s))
            m[:, :n] = full[:, n_s:n_s + n]
        sides.append((mel, ppg, d_l, m))
    (mel_a, p_a, d_la, ma), (mel_b, p_b, d_lb, mb) = sides
    path = path_len = None
    if align == 'dtw':
        ca, cb = _cepstra_launch(mel_a, n_coef, first_coef), _cepstra_launch(mel_b, n_coef, first_coef)
        if mask is not None:
            r = _masked_dtw(ca, cb, _compact_launch(ma, d_la), _compact_launch(mb, d_lb), scale, band, True)
        else:
            r = _dtw_launch(ca, cb, d_la, d_lb, scale, band, True)
        path, path_len = r.path, r.path_len
    c = _content_launch(p_a, p_b, d_la, d_lb, path, path_len, _cmap_device(cmap), min_run, ma, mb, _decode_upload(dec))
    return _CONTENT_WAV(*c, p_a, p_b, d_la, d_lb, path, path_len, ma, mb)


ALIGN_MAX_SEQ = 1024        # vc_align_f32
ALIGN_MAX_CLASSES = 65535
_ALIGN_FIELDS = 'frame_state start end seg_score total n_visited labels'
_ALIGN = namedtuple('alignment', _ALIGN_FIELDS)
_ALIGN_WAV = namedtuple('alignment_wav', _ALIGN_FIELDS + ' ppg n_frames')


def _check_align_ppg(x, what):
    import torch
    if getattr(x, 'ndim', 0) != 3 or min(x.shape) < 1:
        raise ValueError(' - ERROR, {} must be [B, F, C]'.format(what))
    dt = x.dtype if torch.is_tensor(x) else np.asarray(x).dtype
    if dt not in (torch.float32, np.dtype(np.float32)):
        raise ValueError(' - ERROR, {} must be float32, got {}'.format(what, dt))
    B, F, C = (int(v) for v in x.shape)
    if B > 65535 or C > ALIGN_MAX_CLASSES:
        raise ValueError(' - ERROR, {}: at most 65535 rows of at most {} classes (got {} of {})'.format(what, ALIGN_MAX_CLASSES, B, C))
    return B, F, C


def _check_align_seq(seq, n_seq, optional, B, C, what):
    """seq [B, S] int32 and optional None or [B, S] uint8 / bool, each a host array or a device tensor; n_seq as
    _check_counts.  A host seq has its values below the row's count checked against [0, C) (every value of the row
    when the counts live on the device); a device seq is taken as it is: the launch gives a class outside [0, C) the
    score -inf.  Returns (seq, (host counts | None, device counts | None), optional) with host arrays converted."""
    import torch
    if getattr(seq, 'ndim', 0) != 2 or min(seq.shape) < 1 or int(seq.shape[0]) != B:
        raise ValueError(' - ERROR, {}: seq must be [{}, S]'.format(what, B))
    dt = seq.dtype if torch.is_tensor(seq) else np.asarray(seq).dtype
    if dt not in (torch.int32, np.dtype(np.int32)):
        raise ValueError(' - ERROR, {}: seq must be int32, got {}'.format(what, dt))
    S = int(seq.shape[1])
    if S > ALIGN_MAX_SEQ:
        raise ValueError(' - ERROR, {}: at most {} states per utterance (got {})'.format(what, ALIGN_MAX_SEQ, S))
    n = _check_counts(n_seq, B, 0, S, '{}: n_seq'.format(what))
    if not (torch.is_tensor(seq) and seq.is_cuda):
        h = np.ascontiguousarray(seq.cpu().numpy() if torch.is_tensor(seq) else seq)
        used = np.arange(S)[None, :] < (n[0][:, None] if n[0] is not None else S)
        if used.any() and (h[used].min() < 0 or h[used].max() >= C):
            raise ValueError(' - ERROR, {}: seq must hold classes in [0, {})'.format(what, C))
        seq = h
    if optional is not None:
        if getattr(optional, 'ndim', 0) != 2 or tuple(int(v) for v in optional.shape) != (B, S):
            raise ValueError(' - ERROR, {}: optional must be [{}, {}], as seq'.format(what, B, S))
        dt = optional.dtype if torch.is_tensor(optional) else np.asarray(optional).dtype
        if dt not in (torch.uint8, torch.bool, np.dtype(np.uint8), np.dtype(np.bool_)):
            raise ValueError(' - ERROR, {}: optional must be uint8 or bool, got {}'.format(what, dt))
        if not (torch.is_tensor(optional) and optional.is_cuda):
            optional = np.ascontiguousarray((optional.cpu().numpy() if torch.is_tensor(optional) else np.asarray(optional)) != 0, dtype=np.uint8)
    return seq, n, optional


def _check_align_size(B, F, S, what):
    a256 = lambda v: (v + 255) // 256 * 256                         # vc_align_workspace_bytes
    if a256(B * 4) + a256(B * ((F + 15) // 16) * S * 4) >= 2 ** 31:
        raise ValueError(' - ERROR, {}: the moves of {} utterances of {} frames x {} states need 2 GiB or more; align fewer '
                         'utterances per call'.format(what, B, F, S))


def _align_kind(kind, floor, what, kinds=('prob', 'log')):
    if kind not in kinds:
        raise ValueError(" - ERROR, {}: kind must be {}, got {!r}".format(what, ' or '.join((', '.join(map(repr, kinds[:-1])), repr(kinds[-1]))), kind))
    fl = float(floor)
    if not (np.isfinite(fl) and fl > 0.0):
        raise ValueError(' - ERROR, {}: floor must be finite and positive, got {!r}'.format(what, floor))
    return fl


def _pinned_up(h):
    import torch
    return torch.from_numpy(h).pin_memory().to('cuda', non_blocking=True)


def _align_launch(score, seq, opt, d_frames, d_nseq):
    """score: cuda, contiguous float32 [B, F, C]; seq int32 [B, S], opt uint8 [B, S] or None, counts: all on the device.
    The two launches of vc_align_f32 and labels = seq[frame_state].  No host check in here, nothing waited for."""
    import torch
    lib = _vc.lib()
    B, F, C = score.shape
    S = seq.shape[1]
    dev = score.device
    frame_state = torch.empty((B, F), dtype=torch.int32, device=dev)
    bounds = torch.empty((2, B, S), dtype=torch.int32, device=dev)
    n_visited = torch.empty((B,), dtype=torch.int32, device=dev)
    seg_score = torch.empty((B, S), dtype=torch.float32, device=dev)
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    need = lib.vc_align_workspace_bytes(B, F, S)
    if need == 0:
        raise _vc.VCError('vc_align_workspace_bytes refused {} utterances of {} frames x {} states'.format(B, F, S))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    _vc.check(lib.vc_align_f32(_vc.ptr(score), _vc.ptr(seq), _vc.ptr(opt), _vc.ptr(d_frames), _vc.ptr(d_nseq), B, F, S, C,
                               _vc.ptr(frame_state), _vc.ptr(bounds[0]), _vc.ptr(bounds[1]), _vc.ptr(seg_score), _vc.ptr(total),
                               _vc.ptr(n_visited), _vc.ptr(ws), need, _vc.current_stream()))
    labels = torch.where(frame_state >= 0, torch.gather(seq, 1, frame_state.clamp_min(0).long()), frame_state)
    return _ALIGN(frame_state, bounds[0], bounds[1], seg_score, total, n_visited, labels)


def _align_device(seq, n, optional):
    """Uploads (pinned, no wait) whatever of seq / counts / optional is still on the host."""
    import torch
    seq = seq.contiguous() if torch.is_tensor(seq) else _pinned_up(seq)
    if optional is not None:
        optional = (optional.to(torch.uint8).contiguous() if torch.is_tensor(optional) else _pinned_up(optional))
    return seq, optional, _upload_mixed(*n)


def align_batch(ppg, lens, seq, n_seq, optional=None, kind='prob', floor=1e-10):
    """Forced alignment of B utterances (vc_align_f32; the definition is in include/vc_hip.h, "Alignment"): where does each
    phoneme of a KNOWN sequence lie in the frames?  ppg [B, F_max, C] float32 (cuda tensor or numpy array): posteriors
    (kind='prob': the scores are torch.log(ppg.clamp_min(floor)), taken on the device) or ready scores such as
    log-posteriors (kind='log': passed through; finite or -inf).  lens: the frame counts, host integers in [0, F_max] or an
    int32 [B] device tensor.  seq [B, S_max] int32: the expected classes (host array: checked against [0, C); device
    tensor: a class outside gets the score -inf); n_seq: their counts, host integers in [0, S_max] or int32 [B] on the
    device.  optional: None or [B, S_max] uint8 / bool, 1 = the state may be skipped (the silence between two words).
    S_max <= 1,024, B <= 65,535, C <= 65,535, and B * ceil(F_max / 16) * S_max * 4 bytes of moves below 2 GiB.
    Nothing is copied back and the host waits for nothing.  Returns a namedtuple of device tensors: frame_state
    [B, F_max] int32 (the state of every frame, -1 from the count on and for an utterance that cannot be aligned), start,
    end [B, S_max] int32 (first frame, one past the last; -1 for a skipped state), seg_score [B, S_max] float32 (the mean
    score of the state's class over its frames -- with log-posteriors the "goodness of pronunciation"; NaN where start is
    -1), total [B] float32 (-inf: cannot be aligned), n_visited [B] int32, and labels [B, F_max] int32 =
    seq[frame_state] (-1 where frame_state is -1)."""
    import torch
    B, F, C = _check_align_ppg(ppg, 'align_batch: ppg')
    fl = _align_kind(kind, floor, 'align_batch')
    nf = _check_counts(lens, B, 0, F, 'align_batch: lens')
    seq, ns, optional = _check_align_seq(seq, n_seq, optional, B, C, 'align_batch')
    _check_align_size(B, F, int(seq.shape[1]), 'align_batch')
    _need_gpu('align_batch')
    d_seq, d_opt, (d_frames, d_nseq) = _align_device(seq, (nf, ns), optional)
    score = _to_device(ppg, torch.float32)
    if kind == 'prob':
        score = torch.log(score.clamp_min(fl))
    return _align_launch(score, d_seq, d_opt, d_frames, d_nseq)


def _align_wav_front(what, encoder, wav, lens, seq, n_seq, cfg_d, wav_sr, res_type, optional, window_batch, ppg, max_classes,
                     check_size):
    """What align_wav_batch and align_posterior_wav_batch share: the checks, the uploads and the posteriors of
    content_wav_batch's _content_side.  check_size(B, Fout, S, what) is the launch's own size check.  Returns
    (ppg [B, Fout, n_phn], d_seq, d_opt, d_l, d_nseq), all on the device."""
    import torch
    import audio_lib
    import conversion
    if cfg_d is None:
        raise ValueError(' - ERROR, {}: cfg_d (the data-set configuration) is required'.format(what))
    audio_lib._res_params(res_type)
    a = _wav_side(wav, lens, cfg_d, wav_sr, 'wav')
    B = a['B']
    window_batch = int(window_batch)
    if window_batch <= 0:
        raise ValueError(' - ERROR, {}: window_batch must be positive'.format(what))
    plan = conversion.convert_plan(a['h'], cfg_d, 0, 60, True)
    C = int(encoder.cfg_d['n_output'])
    if B > 65535 or C > max_classes:
        raise ValueError(' - ERROR, {}: at most 65535 utterances and {} classes (got {} and {})'.format(what, max_classes, B, C))
    if ppg is not None:
        if _check_align_ppg(ppg, '{}: ppg'.format(what)) != (B, plan.Fout, C):
            raise ValueError(' - ERROR, {}: ppg must be [{}, {}, {}], as convert_batch returns phn_pred for wav'
                             .format(what, B, plan.Fout, C))
    seq, ns, optional = _check_align_seq(seq, n_seq, optional, B, C, what)
    check_size(B, plan.Fout, int(seq.shape[1]), what)
    h_l = np.minimum(plan.n_out, plan.n_clip - plan.n_s)
    if h_l.min() < 1:
        raise ValueError(' - ERROR, {}: every utterance needs at least one frame of its own'.format(what))
    _need_gpu(what)
    d_in, d_len, d_clip, d_win, d_utt, d_true, d_l = _upload_lens(a['h_in'], a['h'], plan.n_clip, plan.win_tab, plan.utt_tab,
                                                                  plan.true_tab, h_l)
    d_seq, d_opt, (d_nseq,) = _align_device(seq, (ns,), optional)
    if ppg is not None:
        ppg = _to_device(ppg, torch.float32)
    _, _, ppg = _content_side(encoder, wav, a, plan, (d_in, d_len, d_clip, d_win.view(-1, 2), d_utt.view(-1, 3), d_true.view(-1, 2)),
                              cfg_d, res_type, window_batch, ppg)
    return ppg, d_seq, d_opt, d_l, d_nseq


def align_wav_batch(encoder, wav, lens, seq, n_seq, cfg_d, wav_sr=None, res_type='kaiser_best', optional=None, window_batch=64,
                    ppg=None):
    """Forced alignment of B WAVEFORMS against their transcripts.  encoder: the phoneme recogniser
    (encoder.encoder_spec_phn).  The posteriors are those of content_wav_batch (its _content_side: the resampler for
    wav_sr, the front-end, convert_batch's window tables with t_s = 0, t_e = 60 and two passes, the encoder in chunks of
    window_batch windows, the stitch), i.e. exactly convert_batch's phn_pred; ppg: such posteriors [B, Fout, n_phn] that
    are already there, instead of running the encoder.  Only frames that come from the waveform are aligned:
    min(n_out, min(n_src, n_e) - n_s) per utterance.  seq, n_seq, optional as in align_batch, which this ends in
    (kind='prob').  Returns align_batch's fields, then ppg [B, Fout, n_phn] and n_frames (int32 [B]), on the device."""
    import torch
    ppg, d_seq, d_opt, d_l, d_nseq = _align_wav_front('align_wav_batch', encoder, wav, lens, seq, n_seq, cfg_d, wav_sr, res_type,
                                                      optional, window_batch, ppg, ALIGN_MAX_CLASSES, _check_align_size)
    r = _align_launch(torch.log(ppg.clamp_min(1e-10)), d_seq, d_opt, d_l, d_nseq)
    return _ALIGN_WAV(*r, ppg, d_l)


FULLSUM_MAX_CLASSES = 4096  # vc_fullsum_f32: the Gamma row lives in LDS
_FULLSUM_FIELDS = 'log_z class_post state_post occupancy feasible'
_FULLSUM = namedtuple('alignment_posterior', _FULLSUM_FIELDS)
_FULLSUM_WAV = namedtuple('alignment_posterior_wav', _FULLSUM_FIELDS + ' ppg n_frames')


def _check_fullsum_size(B, F, S, what):
    if (B * F * S * 4 + 255) // 256 * 256 >= 2 ** 31:               # vc_fullsum_workspace_bytes
        raise ValueError(' - ERROR, {}: the forward rows of {} utterances of {} frames x {} states need 2 GiB or more; pass fewer '
                         'utterances per call'.format(what, B, F, S))


def _check_fullsum_classes(C, what):
    if C > FULLSUM_MAX_CLASSES:
        raise ValueError(' - ERROR, {}: at most {} classes (got {})'.format(what, FULLSUM_MAX_CLASSES, C))


def _fullsum_launch(score, seq, opt, d_frames, d_nseq, return_states=False):
    """score: cuda, contiguous float32 [B, F, C]; seq int32 [B, S], opt uint8 [B, S] or None, counts: all on the device.
    The two launches of vc_fullsum_f32 and feasible = log_z > -inf.  No host check in here, nothing waited for."""
    import torch
    lib = _vc.lib()
    B, F, C = score.shape
    S = seq.shape[1]
    dev = score.device
    log_z = torch.empty((B,), dtype=torch.float32, device=dev)
    class_post = torch.empty((B, F, C), dtype=torch.float32, device=dev)
    state_post = torch.empty((B, F, S), dtype=torch.float32, device=dev) if return_states else None
    occ = torch.empty((B, S), dtype=torch.float32, device=dev)
    need = lib.vc_fullsum_workspace_bytes(B, F, S)
    if need == 0:
        raise _vc.VCError('vc_fullsum_workspace_bytes refused {} utterances of {} frames x {} states'.format(B, F, S))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    _vc.check(lib.vc_fullsum_f32(_vc.ptr(score), _vc.ptr(seq), _vc.ptr(opt), _vc.ptr(d_frames), _vc.ptr(d_nseq), B, F, S, C,
                                 _vc.ptr(log_z), _vc.ptr(class_post), _vc.ptr(state_post), _vc.ptr(occ), _vc.ptr(ws), need,
                                 _vc.current_stream()))
    return _FULLSUM(log_z, class_post, state_post, occ, log_z > float('-inf'))


def _fullsum_score(x, kind, fl):
    import torch
    if kind == 'prob':
        return torch.log(x.clamp_min(fl))
    if kind == 'logits':
        return torch.log_softmax(x, dim=-1)
    return x


def align_posterior_batch(ppg, lens, seq, n_seq, optional=None, kind='prob', floor=1e-10, return_states=False):
    """Full-sum alignment of B utterances (vc_fullsum_f32; the definition is in include/vc_hip.h, "Alignment"): not the best
    path of the transcript through the frames, as align_batch gives it, but the distribution over ALL admissible paths.
    ppg, lens, seq, n_seq, optional and floor as in align_batch; kind 'prob' (the scores are torch.log(ppg.clamp_min(floor))),
    'log' (ready scores, finite or -inf, passed through) or 'logits' (the scores are torch.log_softmax over the classes).
    S_max <= 1,024, B <= 65,535, C <= 4,096, and B * F_max * S_max * 4 bytes of forward rows below 2 GiB.  Nothing is copied
    back and the host waits for nothing.  Returns a namedtuple of device tensors: log_z [B] float32 (the log of the sum
    over the paths of the product of their frames' scores: the transcript's likelihood; -inf: no path), class_post
    [B, F_max, C] float32 (Gamma: the posterior probability that the frame is in a state of the class -- with logits y,
    softmax(y) - class_post is the gradient of -log_z; zero rows from the count on and without a path), state_post
    [B, F_max, S_max] float32 (gamma, per state; None unless return_states), occupancy [B, S_max] float32 (the expected
    number of frames of every state) and feasible [B] bool."""
    import torch
    B, F, C = _check_align_ppg(ppg, 'align_posterior_batch: ppg')
    _check_fullsum_classes(C, 'align_posterior_batch')
    fl = _align_kind(kind, floor, 'align_posterior_batch', ('prob', 'log', 'logits'))
    nf = _check_counts(lens, B, 0, F, 'align_posterior_batch: lens')
    seq, ns, optional = _check_align_seq(seq, n_seq, optional, B, C, 'align_posterior_batch')
    _check_fullsum_size(B, F, int(seq.shape[1]), 'align_posterior_batch')
    _need_gpu('align_posterior_batch')
    d_seq, d_opt, (d_frames, d_nseq) = _align_device(seq, (nf, ns), optional)
    score = _fullsum_score(_to_device(ppg, torch.float32), kind, fl)
    return _fullsum_launch(score, d_seq, d_opt, d_frames, d_nseq, bool(return_states))


def align_posterior_wav_batch(encoder, wav, lens, seq, n_seq, cfg_d, wav_sr=None, res_type='kaiser_best', optional=None,
                              window_batch=64, ppg=None, return_states=False):
    """Full-sum alignment of B WAVEFORMS against their transcripts: align_wav_batch's posteriors (the same front half, ppg
    included) into align_posterior_batch's launch (kind='prob', floor 1e-10).  Returns align_posterior_batch's fields, then
    ppg [B, Fout, n_phn] and n_frames (int32 [B]), on the device."""
    import torch
    ppg, d_seq, d_opt, d_l, d_nseq = _align_wav_front('align_posterior_wav_batch', encoder, wav, lens, seq, n_seq, cfg_d, wav_sr,
                                                      res_type, optional, window_batch, ppg, FULLSUM_MAX_CLASSES, _check_fullsum_size)
    r = _fullsum_launch(torch.log(ppg.clamp_min(1e-10)), d_seq, d_opt, d_l, d_nseq, bool(return_states))
    return _FULLSUM_WAV(*r, ppg, d_l)


# ------------------------------------------------------------------------------------- decoding (csrc/vc_decode.hip)
DECODE_MAX_CLASSES = 128    # vc_decode_f32
DECODE_MAX_DUR = 8
_DECODE_FIELDS = 'frame_class labels seg seg_score total feasible'
_DECODE = namedtuple('decoded', _DECODE_FIELDS)
_DECODE_WAV = namedtuple('decoded_wav', _DECODE_FIELDS + ' ppg n_frames')
_DECODE_ARGS = namedtuple('decode_args', 'trans penalty init final min_dur kind floor')


def _check_decode_size(B, F, C, what):
    if B > 65535 or F > EDIT_MAX or C > DECODE_MAX_CLASSES:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most {} frames of at most {} classes (got {} of {} of {})'
                         .format(what, EDIT_MAX, DECODE_MAX_CLASSES, B, F, C))
    a256 = lambda v: (v + 255) // 256 * 256                         # vc_decode_workspace_bytes
    if a256(B * 4) + a256(B * C * ((F + 3) // 4) * 4) >= 2 ** 31:
        raise ValueError(' - ERROR, {}: the moves of {} utterances of {} frames x {} classes need 2 GiB or more; decode fewer '
                         'utterances per call'.format(what, B, F, C))


def _check_decode_vec(v, shape, what):
    """None, or a float32 array / tensor of the given shape (host: values finite or -inf; device: taken as it is)."""
    import torch
    if v is None:
        return None
    dt = v.dtype if torch.is_tensor(v) else np.asarray(v).dtype
    if tuple(int(n) for n in getattr(v, 'shape', ())) != shape or dt not in (torch.float32, np.dtype(np.float32)):
        raise ValueError(' - ERROR, {} must be float32 {}, got {} {}'.format(what, list(shape), dt, list(getattr(v, 'shape', ()))))
    if torch.is_tensor(v) and v.is_cuda:
        return v.contiguous()
    h = np.ascontiguousarray(v.cpu().numpy() if torch.is_tensor(v) else v)
    if np.isnan(h).any() or (h == np.inf).any():
        raise ValueError(' - ERROR, {} must be finite or -inf'.format(what))
    return h


def _decode_args(trans, penalty, init, final, min_dur, kind, floor, C, what):
    fl = _align_kind(kind, floor, what)
    if isinstance(min_dur, bool) or not isinstance(min_dur, (int, np.integer)) or not 1 <= min_dur <= DECODE_MAX_DUR:
        raise ValueError(' - ERROR, {}: min_dur must be an integer number of frames in [1, {}], got {!r}'.format(what, DECODE_MAX_DUR, min_dur))
    pen = float(penalty)
    if np.isnan(pen) or pen == np.inf:
        raise ValueError(' - ERROR, {}: penalty must be finite or -inf, got {!r}'.format(what, penalty))
    return _DECODE_ARGS(_check_decode_vec(trans, (C, C), '{}: trans'.format(what)), pen, _check_decode_vec(init, (C,), '{}: init'.format(what)),
                        _check_decode_vec(final, (C,), '{}: final'.format(what)), int(min_dur), kind, fl)


def _decode_upload(dec):
    """The host arrays of _decode_args' result go up (pinned, no wait); None stays None."""
    import torch
    if dec is None:
        return None
    up = lambda v: v if v is None or torch.is_tensor(v) else _pinned_up(v)
    return dec._replace(trans=up(dec.trans), init=up(dec.init), final=up(dec.final))


def _decode_trans(dec, C, device):
    """The [C, C] matrix the launch takes: filled with ``penalty`` without a trans, else trans + penalty in one float32 add
    on the device (skipped for 0)."""
    import torch
    if dec.trans is None:
        return torch.full((C, C), dec.penalty, dtype=torch.float32, device=device)
    return dec.trans + dec.penalty if dec.penalty != 0.0 else dec.trans


def _decode_launch(x, d_frames, cmap, dec):
    """x: cuda, contiguous float32 [B, F, C] posteriors or scores (dec.kind); counts, map and dec's arrays on the device.
    The two launches of vc_decode_f32 and labels = class_map[frame_class].  No host check in here, nothing waited for."""
    import torch
    lib = _vc.lib()
    B, F, C = x.shape
    dev = x.device
    score = torch.log(x.clamp_min(dec.floor)) if dec.kind == 'prob' else x
    trans = _decode_trans(dec, C, dev)
    frame_class = torch.empty((B, F), dtype=torch.int32, device=dev)
    out = torch.empty((3, B, F), dtype=torch.int32, device=dev)
    n_seg = torch.empty((B,), dtype=torch.int32, device=dev)
    seg_score = torch.empty((B, F), dtype=torch.float32, device=dev)
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    need = lib.vc_decode_workspace_bytes(B, F, C)
    if need == 0:
        raise _vc.VCError('vc_decode_workspace_bytes refused {} utterances of {} frames x {} classes'.format(B, F, C))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    _vc.check(lib.vc_decode_f32(_vc.ptr(score), _vc.ptr(d_frames), _vc.ptr(trans), _vc.ptr(dec.init), _vc.ptr(dec.final), _vc.ptr(cmap),
                                B, F, C, dec.min_dur, _vc.ptr(frame_class), _vc.ptr(out[0]), _vc.ptr(out[1]), _vc.ptr(out[2]),
                                _vc.ptr(n_seg), _vc.ptr(seg_score), _vc.ptr(total), _vc.ptr(ws), need, _vc.current_stream()))
    labels = frame_class
    if cmap is not None:
        labels = torch.where(frame_class >= 0, cmap[frame_class.clamp_min(0).long()], frame_class)
    return _DECODE(frame_class, labels, _SEG(out[0], out[1], out[2], n_seg), seg_score, total, total > float('-inf'))


def _content_sequence(sequence, decode, B, F, C, what):
    """None for sequence='argmax'; for 'viterbi' the checked arguments of the decoder (decode: a dict or None)."""
    if sequence not in ('argmax', 'viterbi'):
        raise ValueError(" - ERROR, {}: sequence must be 'argmax' or 'viterbi', got {!r}".format(what, sequence))
    if sequence == 'argmax':
        if decode is not None:
            raise ValueError(" - ERROR, {}: decode is for sequence='viterbi'".format(what))
        return None
    kw = dict(trans=None, penalty=0.0, init=None, final=None, min_dur=3, kind='prob', floor=1e-10)
    extra = set(decode or {}) - set(kw)
    if extra:
        raise ValueError(' - ERROR, {}: decode takes {}, got {}'.format(what, sorted(kw), sorted(extra)))
    kw.update(decode or {})
    _check_decode_size(B, F, C, what)
    return _decode_args(C=C, what=what, **kw)


def decode_batch(ppg, lens, trans=None, penalty=0.0, init=None, final=None, min_dur=3, class_map=None, kind='prob', floor=1e-10):
    """Phoneme recognition of B utterances (vc_decode_f32; the definition is in include/vc_hip.h, "Decoding"): the best path
    through a loop of all C classes, with a transition score between two phonemes and at least ``min_dur`` frames per
    phoneme -- a path decision where phn_segments_batch takes the arg-max of every frame and cleans up afterwards.
    ppg [B, F_max, C] float32 (cuda tensor or numpy array): posteriors (kind='prob': the scores are
    torch.log(ppg.clamp_min(floor)), taken on the device) or ready scores (kind='log': passed through; finite or -inf).
    lens: the frame counts, host integers in [0, F_max] or an int32 [B] device tensor.  trans [C, C] float32: trans[i, j] is
    added where a phoneme i ends and a phoneme j begins (phn_transitions builds one from label sequences; i == j: the phoneme
    said twice); None: a matrix filled with ``penalty``; otherwise ``penalty`` (an insertion penalty, <= 0 for fewer
    segments) is added to it on the device.  init, final [C] float32 or None: added at the first / last frame.  class_map:
    None or C integers in [-1, C) (evaluation.class_map).  C <= 128, min_dur in [1, 8], B <= 65,535, F_max <= 16,384.
    Nothing is copied back and the host waits for nothing.  Returns a namedtuple of device tensors: frame_class [B, F_max]
    int32 (the decoded class of every frame; -1 from the count on and for an utterance without a path), labels =
    class_map[frame_class] (-1 kept), seg (labels, start, end [B, F_max] and n_seg [B], as phn_segments_batch returns
    them, so edit_distance_batch takes them: the decoded segments mapped, equal neighbours merged, -1 dropped), seg_score
    [B, F_max] float32 (the mean score of a segment's frames; NaN from n_seg on), total [B] float32 and feasible [B] bool."""
    import torch
    B, F, C = _check_align_ppg(ppg, 'decode_batch: ppg')
    _check_decode_size(B, F, C, 'decode_batch')
    dec = _decode_args(trans, penalty, init, final, min_dur, kind, floor, C, 'decode_batch')
    nf = _check_counts(lens, B, 0, F, 'decode_batch: lens')
    cmap = _check_class_map(class_map, C, 'decode_batch')
    _need_gpu('decode_batch')
    d_frames, = _upload_mixed(nf)
    return _decode_launch(_to_device(ppg, torch.float32), d_frames, _cmap_device(cmap), _decode_upload(dec))


def decode_wav_batch(encoder, wav, lens, cfg_d, wav_sr=None, res_type='kaiser_best', trans=None, penalty=0.0, init=None, final=None,
                     min_dur=3, class_map=None, floor=1e-10, window_batch=64, ppg=None):
    """Phoneme recognition of B WAVEFORMS.  encoder: the phoneme recogniser (encoder.encoder_spec_phn).  The posteriors are
    those of content_wav_batch and align_wav_batch (_content_side with t_s = 0, t_e = 60 and two passes), i.e. exactly
    convert_batch's phn_pred; ppg: such posteriors [B, Fout, n_phn] that are already there.  Only frames that come from the
    waveform are decoded.  The other arguments as in decode_batch, which this ends in (kind='prob').  Returns decode_batch's
    fields, then ppg [B, Fout, n_phn] and n_frames (int32 [B]), on the device."""
    import torch
    import audio_lib
    import conversion
    what = 'decode_wav_batch'
    if cfg_d is None:
        raise ValueError(' - ERROR, {}: cfg_d (the data-set configuration) is required'.format(what))
    audio_lib._res_params(res_type)
    a = _wav_side(wav, lens, cfg_d, wav_sr, 'wav')
    B = a['B']
    window_batch = int(window_batch)
    if window_batch <= 0:
        raise ValueError(' - ERROR, {}: window_batch must be positive'.format(what))
    plan = conversion.convert_plan(a['h'], cfg_d, 0, 60, True)
    C = int(encoder.cfg_d['n_output'])
    _check_decode_size(B, plan.Fout, C, what)
    if ppg is not None:
        if _check_align_ppg(ppg, '{}: ppg'.format(what)) != (B, plan.Fout, C):
            raise ValueError(' - ERROR, {}: ppg must be [{}, {}, {}], as convert_batch returns phn_pred for wav'.format(what, B, plan.Fout, C))
    dec = _decode_args(trans, penalty, init, final, min_dur, 'prob', floor, C, what)
    cmap = _check_class_map(class_map, C, what)
    h_l = np.minimum(plan.n_out, plan.n_clip - plan.n_s)
    if h_l.min() < 1:
        raise ValueError(' - ERROR, {}: every utterance needs at least one frame of its own'.format(what))
    _need_gpu(what)
    d_in, d_len, d_clip, d_win, d_utt, d_true, d_l = _upload_lens(a['h_in'], a['h'], plan.n_clip, plan.win_tab, plan.utt_tab,
                                                                  plan.true_tab, h_l)
    if ppg is not None:
        ppg = _to_device(ppg, torch.float32)
    _, _, ppg = _content_side(encoder, wav, a, plan, (d_in, d_len, d_clip, d_win.view(-1, 2), d_utt.view(-1, 3), d_true.view(-1, 2)),
                              cfg_d, res_type, window_batch, ppg)
    r = _decode_launch(ppg.contiguous(), d_l, _cmap_device(cmap), _decode_upload(dec))
    return _DECODE_WAV(*r, ppg, d_l)


def phn_transitions(seqs, n_seq, n_classes, add=1.0, scale=1.0, allow_repeat=False):
    """A transition matrix for decode_batch from label sequences (host numpy): seqs [N, S] integers in [0, n_classes), n_seq
    [N] their counts.  count[i, j] is the number of times j follows i; the result is
    scale * log((count[i, j] + add) / (row_total[i] + add * C)), float32 [C, C]: with add > 0 every row of exp(result / scale)
    sums to 1.  allow_repeat=False sets the diagonal to -inf: no phoneme follows itself, so a decoded path is determined by
    its frames' classes."""
    C = int(n_classes)
    seqs, n_seq = np.asarray(seqs), np.asarray(n_seq).reshape(-1)
    if C < 1 or seqs.ndim != 2 or seqs.dtype.kind not in 'iu' or n_seq.shape != (seqs.shape[0],) or n_seq.dtype.kind not in 'iu':
        raise ValueError(' - ERROR, phn_transitions: seqs must be integers [N, S], n_seq integers [N] and n_classes positive')
    if len(n_seq) and (n_seq.min() < 0 or n_seq.max() > seqs.shape[1]):
        raise ValueError(' - ERROR, phn_transitions: n_seq must lie in [0, {}]'.format(seqs.shape[1]))
    add, scale = float(add), float(scale)
    if not (np.isfinite(add) and add >= 0.0 and np.isfinite(scale)):
        raise ValueError(' - ERROR, phn_transitions: add must be finite and >= 0, scale finite')
    pair = np.arange(seqs.shape[1] - 1)[None, :] < (n_seq[:, None] - 1) if seqs.shape[1] > 1 else np.zeros((len(seqs), 0), bool)
    i, j = seqs[:, :-1][pair].astype(np.int64), seqs[:, 1:][pair].astype(np.int64)
    if len(i) and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= C):
        raise ValueError(' - ERROR, phn_transitions: seqs must hold classes in [0, {})'.format(C))
    count = np.zeros((C, C), np.float64)
    np.add.at(count, (i, j), 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = scale * np.log((count + add) / (count.sum(1, keepdims=True) + add * C))
    if not allow_repeat:
        out[np.arange(C), np.arange(C)] = -np.inf
    return out.astype(np.float32)


def alignment_min_frames(hop_length, win_length):
    """L of phn_v_from_alignment: the number of frames per segment from which its round trip holds, W/2 // hop + 1."""
    return (int(win_length) // 2) // int(hop_length) + 1


def phn_v_from_alignment(start, end, seq, names, hop_length, n_samples):
    """One utterance's alignment as the (start_sample, end_sample, phn) list that audio_lib.calc_PHN_target consumes.
    start, end: the utterance's rows of align_batch's result, downloaded (host integers, -1 = the state was skipped: it
    is left out); seq: its expected classes; names[c]: the phoneme name of class c; n_samples: the samples of the
    waveform (the aligned frame count must be the front-end's F = 1 + n_samples // hop_length).

    Where the sample boundaries go.  calc_PHN_target gives frame i the window [i hop - H, i hop + H) (H = win_length / 2,
    win_length even), takes as "current" the first segment that ends after the window's start, and picks the NEXT segment
    instead iff the window overlaps that one strictly more -- it compares these two only.  For a window that straddles
    one boundary b, with both neighbours reaching beyond the window, the overlaps are b - (i hop - H) and (i hop + H) - b:
    the next segment wins iff b < i hop.  A state whose frames are [st, en) must keep frame en - 1 and lose frame en, so
    (en - 1) hop <= b < en hop.  This helper puts b = en hop - h2, h2 = ceil(hop / 2): the middle of that range.  The
    first segment starts at sample 0 and the last one ends at n_samples: the list labels the waveform, nothing outside.

    How long segments must be.  Number the visited segments k = 0 .. n-1, b_k the end of k, frames [st_k, en_k), len_k
    frames.  Frame i of segment k is labelled k when
    (1) "current" is k - 1 or k, i.e. segment k - 2 ends at or before the window's start even for i = st_k:
        b_{k-2} = st_{k-1} hop - h2 <= st_k hop - H, i.e. len_{k-1} hop >= H - h2;
    (2) with "current" = k the comparison keeps k.  If the window ends inside k the next overlap is not positive.  Else
        k overlaps by b_k - (i hop - H) and k + 1 by at most (i hop + H) - b_k, and b_k >= i hop holds for i <= en_k - 1.
        Only the FIRST segment can start after the window's start (sample 0 against a negative i hop - H): then its
        overlap is b_0 = len_0 hop - h2 against at most i hop + H - b_0, largest at i = len_0 - 1, which asks
        len_0 hop >= H + 2 h2 - hop;
    (3) with "current" = k - 1 the comparison moves on to k.  The overlap of k - 1 is at most b_{k-1} - (i hop - H)
        <= H - h2 (largest at i = st_k).  If k reaches beyond the window its overlap is (i hop + H) - b_{k-1} >= H + h2.
        Otherwise it is the whole of k, which must be STRICTLY more than H - h2: len_k hop >= H - h2 + 1 for an inner
        segment; the LAST segment ends at n_samples >= (F - 1) hop, so it holds at least (len_k - 1) hop + h2 samples,
        which asks len_k hop >= H + hop - 2 h2 + 1.
    hop - 2 h2 is 0 or -1, so all of these hold when len_k hop >= H + 1 for every visited segment: the round trip
        calc_PHN_target(y, phn_v_from_alignment(...), name -> class, hop, W) == seq[frame_state]
    holds when every visited segment lasts at least L = H // hop + 1 frames (alignment_min_frames; 3 for hop 80, W 400).
    The edges set L: inner segments get by with (3)'s H - h2 + 1 samples.  At L - 1 it fails: (L - 1) hop <= H, and with
    n_samples = (F - 1) hop the last segment holds (L - 2) hop + h2 <= H - h2 samples for an even hop -- no longer
    strictly more than its left neighbour's overlap, so its first frame keeps the neighbour's label
    (tests/test_align_cpu.py runs the case)."""
    start, end, seq = (np.asarray(v).reshape(-1) for v in (start, end, seq))
    hop, n_samples = int(hop_length), int(n_samples)
    if hop < 1 or n_samples < 1:
        raise ValueError(' - ERROR, phn_v_from_alignment: hop_length and n_samples must be positive')
    if not len(start) == len(end) == len(seq):
        raise ValueError(' - ERROR, phn_v_from_alignment: start, end and seq must have one entry per state')
    vis = [s for s in range(len(seq)) if start[s] >= 0]
    if not vis:
        return []
    h2 = (hop + 1) // 2
    out = []
    for n, s in enumerate(vis):
        a = 0 if n == 0 else int(start[s]) * hop - h2
        b = n_samples if n == len(vis) - 1 else int(end[s]) * hop - h2
        out.append((a, b, names[int(seq[s])]))
    return out


# ---------------------------------------------------------------------------------------------------- intelligibility
STOI_SR = 10000             # vc_stoi_*: the rate the scores are defined at
STOI_W = 256
STOI_HOP = 128
STOI_NFFT = 512
STOI_SEG = 30               # frames per segment
STOI_MAX_BANDS = 32
_STOI = namedtuple('stoi', 'score n_segments n_kept seg')
_SI_SDR = namedtuple('si_sdr', 'si_sdr valid')
_STOI_BANDS = {}


def stoi_frames(n):
    """The frames of n samples under STOI's framing (MATLAB's): starts i * 128 for every i * 128 < n - 256."""
    n = int(n)
    return 0 if n <= STOI_W else (n - STOI_W + STOI_HOP - 1) // STOI_HOP


def stoi_bands(fs=10000, n_fft=512, n_bands=15, f_min=150.0):
    """The one-third-octave band table of STOI, int32 [n_bands, 2]: band j takes the bins [lo_j, hi_j) of an n_fft-point
    transform at rate fs, lo_j = argmin |f - f_min 2^((2j - 1) / 6)|, hi_j = argmin |f - f_min 2^((2j + 1) / 6)| over
    f = linspace(0, fs, n_fft + 1)[: n_fft // 2 + 1].  Host only.  The defaults give the lower edges 7 9 11 14 17 22 27 34
    43 55 69 87 109 138 174 and the last upper edge 219."""
    for v, name in ((fs, 'fs'), (n_fft, 'n_fft'), (n_bands, 'n_bands')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(' - ERROR, stoi_bands: {} must be a positive integer, got {!r}'.format(name, v))
    if isinstance(f_min, bool) or not isinstance(f_min, (int, float, np.integer, np.floating)) or not 0.0 < f_min < float('inf'):
        raise ValueError(' - ERROR, stoi_bands: f_min must be a positive number, got {!r}'.format(f_min))
    if n_fft % 2:
        raise ValueError(' - ERROR, stoi_bands: n_fft must be even, got {!r}'.format(n_fft))
    f = np.linspace(0.0, float(fs), int(n_fft) + 1)[:int(n_fft) // 2 + 1]
    j = np.arange(int(n_bands), dtype=np.float64)
    lo = np.argmin(np.abs(f[None, :] - (float(f_min) * 2.0 ** ((2.0 * j - 1.0) / 6.0))[:, None]), axis=1)
    hi = np.argmin(np.abs(f[None, :] - (float(f_min) * 2.0 ** ((2.0 * j + 1.0) / 6.0))[:, None]), axis=1)
    return np.stack([lo, hi], axis=1).astype(np.int32)


def _stoi_bands_device():
    import torch
    t = _STOI_BANDS.get('default')
    if t is None:
        t = _STOI_BANDS['default'] = torch.from_numpy(stoi_bands()).pin_memory().to('cuda', non_blocking=True)
    return t


def _check_pair(what, ref, deg, lens, allow_device_lens=True):
    """Host checks of a time-aligned pair: (B, Lmax).  ValueError before the GPU is touched."""
    import torch
    for v, name in ((ref, 'ref'), (deg, 'deg')):
        if getattr(v, 'ndim', 0) != 2 or min(v.shape) < 1:
            raise ValueError(' - ERROR, {}: {} must be [B, Lmax]'.format(what, name))
    if tuple(ref.shape) != tuple(deg.shape):
        raise ValueError(' - ERROR, {}: ref and deg are time-aligned and must have one shape, got {} and {}'.format(
            what, tuple(ref.shape), tuple(deg.shape)))
    B, Lmax = int(ref.shape[0]), int(ref.shape[1])
    if B > 65535 or Lmax > 2 ** 30:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most 2^30 samples'.format(what))
    if lens is not None and torch.is_tensor(lens) and lens.is_cuda:
        if not allow_device_lens:
            raise ValueError(' - ERROR, {}: lens must be host integers when the pair is resampled'.format(what))
        if lens.dtype != torch.int32 or tuple(lens.shape) != (B,):
            raise ValueError(' - ERROR, {}: lens on the device must be int32 [{}]'.format(what, B))
    elif lens is not None:
        h = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > Lmax:
            raise ValueError(' - ERROR, {}: lens must be {} integers in [0, {}]'.format(what, B, Lmax))
    return B, Lmax


def _pair_device(x):
    import torch
    x = _to_device(x, torch.float32)
    if x.shape[0] == 1:                                             # (the stride of a one-row tensor is arbitrary)
        x = x.as_strided(x.shape, (x.shape[1], 1))
    return x


def _stoi_launch(ref, deg, d_len, mode, ratio, return_segments):
    """The five launches of stoi_batch on validated device tensors at 10 kHz; no host check, copy or wait in here."""
    import torch
    lib, st = _vc.lib(), _vc.current_stream()
    B, Lmax = ref.shape
    dev = ref.device
    Fmax = max(stoi_frames(Lmax), 1)
    Mmax = max(Fmax - 1, 1)
    Smax = max(Mmax - STOI_SEG + 1, 1)
    bands = _stoi_bands_device()
    nb = int(bands.shape[0])
    energy = torch.empty((B, Fmax), dtype=torch.float32, device=dev)
    n_frames = torch.empty((B,), dtype=torch.int32, device=dev)
    index = torch.empty((B, Fmax), dtype=torch.int32, device=dev)
    n_kept = torch.empty((B,), dtype=torch.int32, device=dev)
    T = torch.empty((2, B, Mmax, nb), dtype=torch.float32, device=dev)
    seg = torch.empty((B, Smax), dtype=torch.float32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    n_seg = torch.empty((B,), dtype=torch.int32, device=dev)
    _vc.check(lib.vc_stoi_energy_f32(_vc.ptr(ref), _vc.ptr(d_len), B, Lmax, Lmax, _vc.ptr(energy), _vc.ptr(n_frames), Fmax, st))
    _vc.check(lib.vc_stoi_keep_f32(_vc.ptr(energy), _vc.ptr(n_frames), B, Fmax, ratio, _vc.ptr(index), _vc.ptr(n_kept), st))
    _vc.check(lib.vc_stoi_bands_f32(_vc.ptr(ref), _vc.ptr(deg), B, Lmax, Lmax, _vc.ptr(index), _vc.ptr(n_kept), Fmax, _vc.ptr(bands),
                                    nb, _vc.ptr(T), Mmax, st))
    _vc.check(lib.vc_stoi_score_f32(_vc.ptr(T), _vc.ptr(n_kept), B, Fmax, Mmax, nb, mode, _vc.ptr(seg), Smax, _vc.ptr(score),
                                    _vc.ptr(n_seg), st))
    return _STOI(score, n_seg, n_kept, seg if return_segments else None)


def stoi_batch(ref, deg, lens=None, wav_sr=10000, extended=False, dyn_range=40.0, res_type='kaiser_best', return_segments=False):
    """Short-time objective intelligibility of a TIME-ALIGNED ragged batch: clean reference against processed signal (the
    output of enhance.denoise_batch, of a resampler, of audio_lib.stft_filter_batch, ...).  STOI (Taal et al. 2011), or
    ESTOI (Jensen & Taal 2016) with ``extended``; include/vc_hip.h, "Intelligibility", defines every step.

    ref, deg [B, Lmax] float32 (numpy or tensors) and ONE ``lens`` for both, because the pair is aligned: host integers or,
    at 10 kHz, an int32 [B] device tensor (None = all Lmax).  The scores are defined at 10 kHz.  With another ``wav_sr``
    both sides go through audio_lib.resample_batch first (``res_type``): that resampler is this project's (librosa's
    Kaiser-windowed sinc), NOT the polyphase filter of the papers' MATLAB code, so figures differ slightly from a published
    implementation's, and its output lengths come back on the host, so ``lens`` must be host integers, each above 0.
    dyn_range: frames of the reference more than this many dB below its loudest frame are removed from both signals.
    Returns a namedtuple of device tensors: score [B] float32; n_segments [B] int32, the 30-frame segments averaged (0: the
    utterance is too short or silent and its score is 0, not NaN); n_kept [B] int32, the frames that survived the removal;
    seg [B, S] float32, the per-segment values, zeros beyond n_segments (None unless return_segments).
    After the resampling nothing is copied back and the host waits for nothing.  At most 16,384 frames (209 s) per
    utterance."""
    import torch
    import audio_lib
    what = 'stoi_batch'
    wav_sr = audio_lib._check_rate(wav_sr, 'wav_sr')
    res = wav_sr != STOI_SR
    B, Lmax = _check_pair(what, ref, deg, lens, allow_device_lens=not res)
    if isinstance(dyn_range, bool) or not isinstance(dyn_range, (int, float, np.integer, np.floating)) or not 0.0 < dyn_range <= 300.0:
        raise ValueError(' - ERROR, {}: dyn_range must be a number of dB in (0, 300], got {!r}'.format(what, dyn_range))
    ratio = float(np.float32(10.0 ** (-float(dyn_range) / 10.0)))
    if not 0.0 < ratio < 1.0:
        raise ValueError(' - ERROR, {}: dyn_range {!r} leaves no float32 ratio inside (0, 1)'.format(what, dyn_range))
    if res:
        audio_lib._res_params(res_type)
        if lens is not None and np.asarray(lens.cpu() if torch.is_tensor(lens) else lens).min() <= 0:
            raise ValueError(' - ERROR, {}: every length must be above 0 when the pair is resampled'.format(what))
    L10 = audio_lib.resample_len(Lmax, wav_sr, STOI_SR) if res else Lmax
    if stoi_frames(L10) > MAX_FRAMES:
        raise ValueError(' - ERROR, {}: {} samples at 10 kHz give more than {} frames; score shorter stretches'.format(
            what, L10, MAX_FRAMES))
    _need_gpu(what)
    ref, deg = _pair_device(ref), _pair_device(deg)
    if res:
        h = None if lens is None else np.asarray(lens.cpu() if torch.is_tensor(lens) else lens, dtype=np.int64)
        ref, h10 = audio_lib.resample_batch(ref, h, sr_in=wav_sr, sr_out=STOI_SR, res_type=res_type)
        deg, _ = audio_lib.resample_batch(deg, h, sr_in=wav_sr, sr_out=STOI_SR, res_type=res_type)
        lens = h10
    d_len = None if lens is None else audio_lib._int32_device(lens, B, 'lens')
    return _stoi_launch(ref, deg, d_len, 1 if extended else 0, ratio, bool(return_segments))


def si_sdr_batch(ref, deg, lens=None, zero_mean=True):
    """Scale-invariant signal-to-distortion ratio (Le Roux et al. 2019) of a time-aligned ragged batch, in dB:
    10 log10(|a x|^2 / |a x - y|^2) with a = <y, x> / <x, x> over each utterance's first ``len`` samples; with zero_mean
    each signal loses its own mean first.  ref, deg [B, Lmax] float32 (numpy or tensors); lens: host integers or an int32
    [B] device tensor (None = all Lmax).  Returns a namedtuple of device tensors (si_sdr [B] float32, valid [B] uint8):
    valid 0 and si_sdr 0 for an empty utterance or a reference of zeros; +inf when deg is a multiple of ref, -inf when deg
    holds nothing of it.  The sums are float64 on the device; nothing is copied back and the host waits for nothing."""
    import torch
    import audio_lib
    what = 'si_sdr_batch'
    B, Lmax = _check_pair(what, ref, deg, lens)
    if not isinstance(zero_mean, (bool, np.bool_)):
        raise ValueError(' - ERROR, {}: zero_mean must be True or False, got {!r}'.format(what, zero_mean))
    _need_gpu(what)
    ref, deg = _pair_device(ref), _pair_device(deg)
    d_len = None if lens is None else audio_lib._int32_device(lens, B, 'lens')
    out = torch.empty((B,), dtype=torch.float32, device=ref.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=ref.device)
    _vc.check(_vc.lib().vc_si_sdr_f32(_vc.ptr(ref), _vc.ptr(deg), _vc.ptr(d_len), B, Lmax, Lmax, int(bool(zero_mean)), _vc.ptr(out),
                                      _vc.ptr(valid), _vc.current_stream()))
    return _SI_SDR(out, valid)
