"""Spectral mapping on the MI355X: a conversion that is fitted in seconds from a few parallel sentences, with no encoder
and no decoder (Toda, Black and Tokuda 2007; the front of sprocket's DIFFVC).

A joint-density Gaussian mixture over pairs (x, y) of source and target features -- n cepstra and their regression over
+-2 frames, D = 2 n; every dimension of every component carries a 2 x 2 covariance -- is fitted by EM along the DTW paths
of parallel utterances.  Conversion forms, per source frame, the conditional precisions P and precision-weighted means R of
the target's statics and deltas, and maximum-likelihood parameter generation (MLPG) solves for the static trajectory that
agrees best with both.  The converted cepstra become the gain of the differential filter (audio_lib.stft_filter_batch).

  fit(feat_src, lens_src, feat_tgt, lens_tgt, path, path_len, n_components, n_iter, ...)  -> (JDGMM, trace [n_iter])
  fit_wav(wav_src, lens_src, wav_tgt, lens_tgt, cfg_d, n_coef, n_realign, ...)            -> (JDGMM, trace)
  map_batch(model, feat, lens, mixture)                                                   -> (P, R, mmse, best)
  mlpg_batch(P, R, lens)                                                                  -> (y [B, F, n], flags [B])
  convert_cepstra_batch(model, cep, lens, mixture, mlpg)                                  -> cep_pred [B, F, n]
  cepstra_gain_batch(cep_pred, cep_src, n_frames, cfg_d, alpha, max_boost_db, max_cut_db) -> gain [B, F, bins]

Definitions: include/vc_hip.h, "Spectral mapping"; DESIGN.md section 32.  Every check is made on the host before the first
launch; after that nothing is copied to the host and the host waits for nothing.  All arithmetic runs in
csrc/vc_mapping.hip; the E-step never stores the [cells, components] posteriors.  There is no CPU path.
"""
from collections import namedtuple

import numpy as np

import _vc
import evaluation as ev
import speaker

MAX_COMPONENTS = 256
MAX_DIM = 64
MAX_COEF = 32
MAX_PATH = 2 ** 24
MLPG_MAX_FRAMES = 2 ** 20
JD_TILE = 32                    # vc_jd_tile(): cells per E-step tile, frames per workgroup of the map launch
GAIN_MAX_MELS = 128
GAIN_MAX_BINS = 2049
MIXTURES = {'soft': 0, 'best': 1}

JDGMM = namedtuple('jdgmm', 'w mu_x mu_y var_x var_y cov_xy')
_STATS = namedtuple('jd_stats', 'N S L')
_MAP = namedtuple('jd_map', 'P R mmse best')
_MLPG = namedtuple('mlpg', 'y flags')
_BINS = {}


# ------------------------------------------------------------------------------------------------------------- host checks
def _check_model(model, D, what):
    if not (isinstance(model, tuple) and len(model) == 6):
        raise ValueError(' - ERROR, {}: model must be a JDGMM(w, mu_x, mu_y, var_x, var_y, cov_xy)'.format(what))
    for t, name in zip(model, JDGMM._fields):
        if not speaker._is_f32(t):
            raise ValueError(' - ERROR, {}: model.{} must be float32'.format(what, name))
    w = model[0]
    M = int(w.shape[0]) if getattr(w, 'ndim', 0) == 1 else 0
    if not 1 <= M <= MAX_COMPONENTS:
        raise ValueError(' - ERROR, {}: model.w must be [M] with 1 <= M <= {}'.format(what, MAX_COMPONENTS))
    for t, name in zip(model[1:], JDGMM._fields[1:]):
        if tuple(t.shape) != (M, D):
            raise ValueError(' - ERROR, {}: model.{} must be [M, D] = [{}, {}] like the features, got {}'.format(what, name, M, D,
                                                                                                              tuple(t.shape)))
    return M


def _check_even(D, what):
    if D % 2:
        raise ValueError(' - ERROR, {}: the features are statics and deltas, D must be even (got {})'.format(what, D))
    return D // 2


def _check_mixture(mixture, what):
    if mixture not in MIXTURES:
        raise ValueError(" - ERROR, {}: mixture must be 'soft' or 'best', got {!r}".format(what, mixture))
    return MIXTURES[mixture]


def _check_path(path, path_len, B, Fa, Fb, what):
    """None, or (max_path) of a pair of int32 arrays [B, max_path, 2] and [B] -- numpy or cuda, as dtw_batch returns them."""
    if (path is None) != (path_len is None):
        raise ValueError(' - ERROR, {}: pass path and path_len together or neither'.format(what))
    if path is None:
        return 0
    if getattr(path, 'ndim', 0) != 3 or int(path.shape[0]) != B or int(path.shape[2]) != 2 or int(path.shape[1]) < 1:
        raise ValueError(' - ERROR, {}: path must be [{}, max_path, 2]'.format(what, B))
    if tuple(path_len.shape) != (B,):
        raise ValueError(' - ERROR, {}: path_len must be [{}]'.format(what, B))
    for t, name in ((path, 'path'), (path_len, 'path_len')):
        if str(t.dtype) not in ('torch.int32', 'int32'):
            raise ValueError(' - ERROR, {}: {} must be int32, got {}'.format(what, name, t.dtype))
    if int(path.shape[1]) > MAX_PATH:
        raise ValueError(' - ERROR, {}: a path holds at most 2^24 cells'.format(what))
    return int(path.shape[1])


def _i32_dev(t):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32))
    return t.to(device='cuda', dtype=torch.int32).contiguous()


def _model_to_device(model):
    return JDGMM(*(speaker._f32(t) for t in model))


# ---------------------------------------------------------------------------------------------------------------- launches
def table_floats(M, D):
    return int(_vc.lib().vc_jd_table_floats(int(M), int(D)))


def workspace_size(M, D):
    """vc_jd_workspace_size: host arithmetic."""
    return int(_vc.lib().vc_jd_workspace_size(int(M), int(D)))


def mlpg_workspace_size(B, F, n):
    return int(_vc.lib().vc_mlpg_workspace_size(int(B), int(F), int(n)))


def _prepare_launch(model):
    import torch
    M, D = model.mu_x.shape
    table = torch.empty((table_floats(M, D),), dtype=torch.float32, device=model.mu_x.device)
    _vc.check(_vc.lib().vc_jd_prepare_f32(*(_vc.ptr(t) for t in model), M, D, _vc.ptr(table), _vc.current_stream()))
    return table


def _accumulate_launch(fa, fb, d_la, d_lb, path, path_len, table, M, ws=None):
    import torch
    B, Fa, D = fa.shape
    dev = fa.device
    st = _STATS(torch.empty((M,), dtype=torch.float64, device=dev), torch.empty((5, M, D), dtype=torch.float64, device=dev),
                torch.empty((2,), dtype=torch.float64, device=dev))
    if ws is None:
        ws = torch.empty((workspace_size(M, D),), dtype=torch.uint8, device=dev)
    _vc.check(_vc.lib().vc_jd_accumulate_f32(_vc.ptr(fa), _vc.ptr(fb), _vc.ptr(d_la), _vc.ptr(d_lb), _vc.ptr(path), _vc.ptr(path_len), B,
                                             Fa, fb.shape[1], 0 if path is None else path.shape[1], D, _vc.ptr(table), M, _vc.ptr(st.N),
                                             _vc.ptr(st.S), _vc.ptr(st.L), _vc.ptr(ws), ws.numel(), _vc.current_stream()))
    return st


def _update_launch(st, model, floor_x, floor_y, rho_max, min_count):
    import torch
    M, D = model.mu_x.shape
    out = JDGMM(torch.empty((M,), dtype=torch.float32, device=model.mu_x.device), *(torch.empty_like(model.mu_x) for _ in range(5)))
    _vc.check(_vc.lib().vc_jd_update_f32(_vc.ptr(st.N), _vc.ptr(st.S), M, D, *(_vc.ptr(t) for t in model[1:]), _vc.ptr(floor_x),
                                         _vc.ptr(floor_y), float(rho_max), float(min_count), *(_vc.ptr(t) for t in out),
                                         _vc.current_stream()))
    return out


def _map_launch(feat, d_len, table, M, mixture, want_mmse=True):
    import torch
    B, F, D = feat.shape
    P, R = torch.empty_like(feat), torch.empty_like(feat)
    mmse = torch.empty_like(feat) if want_mmse else None
    best = torch.empty((B, F), dtype=torch.int32, device=feat.device)
    _vc.check(_vc.lib().vc_jd_map_f32(_vc.ptr(feat), _vc.ptr(d_len), B, F, D, _vc.ptr(table), M, mixture, _vc.ptr(P), _vc.ptr(R),
                                      _vc.ptr(mmse), _vc.ptr(best), _vc.current_stream()))
    return _MAP(P, R, mmse, best)


def _mlpg_launch(P, R, d_len):
    import torch
    B, F, D = P.shape
    n = D // 2
    y = torch.empty((B, F, n), dtype=torch.float32, device=P.device)
    flags = torch.empty((B,), dtype=torch.int32, device=P.device)
    ws = torch.empty((mlpg_workspace_size(B, F, n),), dtype=torch.uint8, device=P.device)
    _vc.check(_vc.lib().vc_mlpg_f32(_vc.ptr(P), _vc.ptr(R), _vc.ptr(d_len), B, F, n, _vc.ptr(y), _vc.ptr(flags), _vc.ptr(ws), ws.numel(),
                                    _vc.current_stream()))
    return _MLPG(y, flags)


def _gain_launch(cep_pred, cep_src, d_nf, d_dct, d_i0, d_w, alpha, db_scale, boost, cut):
    import torch
    B, F, n = cep_pred.shape
    nb = d_i0.shape[0]
    gain = torch.empty((B, F, nb), dtype=torch.float32, device=cep_pred.device)
    _vc.check(_vc.lib().vc_cep_gain_f32(_vc.ptr(cep_pred), _vc.ptr(cep_src), _vc.ptr(d_nf), B, F, n, _vc.ptr(d_dct), d_dct.shape[1],
                                        _vc.ptr(d_i0), _vc.ptr(d_w), nb, alpha, db_scale, boost, cut, _vc.ptr(gain),
                                        _vc.current_stream()))
    return gain


# ------------------------------------------------------------------------------------------------------------------ tables
def bin_table(mel_fb):
    """(i0 int32 [bins], w float32 [bins]) from a mel filterbank [n_mels, bins]: a bin's filter weights normalised to sum 1
    are (1 - w) on band i0 and w on band i0 + 1.  Every bin must have at most two non-zero bands and they must be adjacent
    (ValueError otherwise); a bin without any takes the band whose peak lies nearest.  Host only."""
    fb = np.asarray(mel_fb, dtype=np.float64)
    n_mels, nb = fb.shape
    if n_mels < 2:
        raise ValueError(' - ERROR, bin_table: the filterbank needs at least two bands')
    peak = fb.argmax(axis=1)
    i0, w = np.zeros(nb, np.int32), np.zeros(nb, np.float32)
    for k in range(nb):
        nz = np.flatnonzero(fb[:, k] > 0.0)
        if len(nz) == 0:
            nz = np.array([int(np.abs(peak - k).argmin())])
        if len(nz) > 2 or (len(nz) == 2 and nz[1] != nz[0] + 1):
            raise ValueError(' - ERROR, bin_table: bin {} of the filterbank has weight on the bands {}: the gain interpolates '
                             'between two adjacent bands only'.format(k, nz.tolist()))
        if len(nz) == 2:
            i0[k], w[k] = nz[0], fb[nz[1], k] / (fb[nz[0], k] + fb[nz[1], k])
        elif nz[0] <= n_mels - 2:
            i0[k], w[k] = nz[0], 0.0
        else:
            i0[k], w[k] = n_mels - 2, 1.0
    return i0, w


def gain_tables(cfg_d):
    """(i0, w) of bin_table for the front-end of cfg_d (audio_lib.host_tables' filterbank); cached.  Host only."""
    import audio_lib
    n_fft = int(cfg_d['n_fft'] or cfg_d['win_length'])
    key = (int(cfg_d['sample_rate']), n_fft, int(cfg_d['n_mels']))
    t = _BINS.get(key)
    if t is None:
        t = _BINS[key] = bin_table(audio_lib.host_tables(key[0], key[1], key[2], 1)[0])
    return t


def db_scale(cfg_d):
    """Normalised mel units to power dB: the front-end's mel is M_dB_norm_factor * 20 log10(power)."""
    return 1.0 / (2.0 * float(cfg_d['M_dB_norm_factor']))


# ------------------------------------------------------------------------------------------------------------------ public
def _init_means(fa, fb, path, d_plen, M):
    """The pairs at the cells floor((m + 1/2) n / M) of the concatenated paths, on the device (n is known there only)."""
    import torch
    B = fa.shape[0]
    plen = d_plen.to(torch.int64)
    if path is not None:
        plen = plen.clamp(0, path.shape[1])
    ends = torch.cumsum(plen, 0)
    pos = ((2 * torch.arange(M, dtype=torch.int64, device=fa.device) + 1) * ends[-1]) // (2 * M)
    b = torch.searchsorted(ends, pos, right=True).clamp(max=B - 1)
    p = (pos - (ends[b] - plen[b])).clamp(min=0)
    if path is None:
        i = j = p
    else:
        cell = path[b, p.clamp(max=path.shape[1] - 1)].to(torch.int64)
        i, j = cell[:, 0], cell[:, 1]
    i, j = i.clamp(0, fa.shape[1] - 1), j.clamp(0, fb.shape[1] - 1)
    return fa[b, i].contiguous(), fb[b, j].contiguous()


def _fit_device(fa, fb, d_la, d_lb, path, d_plen, M, n_iter, var_floor, rho_max, min_count, ws=None):
    """EM on device tensors; no host check, copy or wait in here.  d_plen: path_len, or min(len_a, len_b) without a path."""
    import torch
    D, dev = fa.shape[2], fa.device
    plen = d_plen if path is not None else None
    if ws is None:
        ws = torch.empty((max(workspace_size(M, D), workspace_size(1, D)),), dtype=torch.uint8, device=dev)
    # the global variances: one component, means 0, variances 1, covariance 0 -- gamma = 1 exactly
    one, zero = torch.ones((1, D), dtype=torch.float32, device=dev), torch.zeros((1, D), dtype=torch.float32, device=dev)
    unit = JDGMM(one[0, :1].contiguous(), zero, zero, one, one, zero)
    st = _accumulate_launch(fa, fb, d_la, d_lb, path, plen, _prepare_launch(unit), 1, ws=ws)
    g = _update_launch(st, unit, zero[0], zero[0], 0.0, 0.0)
    floor_x, floor_y = (g.var_x[0] * var_floor).contiguous(), (g.var_y[0] * var_floor).contiguous()
    mu_x, mu_y = _init_means(fa, fb, path, d_plen, M)
    model = JDGMM(torch.full((M,), 1.0 / M, dtype=torch.float32, device=dev), mu_x, mu_y, g.var_x.expand(M, D).contiguous(),
                  g.var_y.expand(M, D).contiguous(), torch.zeros((M, D), dtype=torch.float32, device=dev))
    trace = torch.empty((n_iter,), dtype=torch.float64, device=dev)
    for it in range(n_iter):
        st = _accumulate_launch(fa, fb, d_la, d_lb, path, plen, _prepare_launch(model), M, ws=ws)
        trace[it] = st.L[0] / st.L[1]
        model = _update_launch(st, model, floor_x, floor_y, rho_max, min_count)
    return model, trace


def _fit_args(n_components, n_iter, var_floor, rho_max, min_count, what):
    M = speaker._check_count(n_components, what + ': n_components', 1, MAX_COMPONENTS)
    n_iter = speaker._check_count(n_iter, what + ': n_iter', 1, 10 ** 6)
    var_floor = speaker._check_pos(var_floor, what + ': var_floor', 0.0, strict=True)
    rho_max = speaker._check_pos(rho_max, what + ': rho_max')
    if not rho_max < 1.0:
        raise ValueError(' - ERROR, {}: rho_max must lie in [0, 1), got {!r}'.format(what, rho_max))
    return M, n_iter, var_floor, rho_max, speaker._check_pos(min_count, what + ': min_count')


def fit(feat_src, lens_src, feat_tgt, lens_tgt, path=None, path_len=None, n_components=32, n_iter=20, var_floor=1e-4, rho_max=0.99,
        min_count=1.0):
    """EM for the joint-density mixture on the cells of B parallel pairs: feat_src [B, Fa, D], feat_tgt [B, Fb, D] float32
    (speaker.features_batch(deltas=True, cmn=False)); lens: host integers.  path [B, max_path, 2] int32 with path_len [B]
    as evaluation.dtw_batch(return_path=True) returns them (numpy or cuda), or both None for the cells (p, p).

    Initialisation is deterministic, without k-means: the means are the pairs at the cells floor((m + 1/2) n / M) of the
    concatenated paths, the variances the global ones (one E-step with a single component), cov_xy = 0, weights uniform.
    var_floor: the floor of every variance as a fraction of the global one; rho_max: the bound of every correlation, so that
    det > 0; min_count: a component that gathers less keeps its means, variances and covariance.  Every iteration is
    vc_jd_prepare_f32, vc_jd_accumulate_f32, vc_jd_update_f32.  Returns (JDGMM, trace [n_iter] float64): trace[i] is the mean
    log-likelihood per cell BEFORE update i.  All on the device."""
    what = 'mapping.fit'
    B, Fa, D = speaker._check_feat(feat_src, what + ': feat_src')
    Bb, Fb, Db = speaker._check_feat(feat_tgt, what + ': feat_tgt')
    if (Bb, Db) != (B, D):
        raise ValueError(' - ERROR, {}: feat_src {} and feat_tgt {} must agree in B and D'.format(what, tuple(feat_src.shape),
                                                                                               tuple(feat_tgt.shape)))
    h_a, h_b = ev._check_lens(lens_src, B, Fa, what + ': lens_src'), ev._check_lens(lens_tgt, B, Fb, what + ': lens_tgt')
    _check_path(path, path_len, B, Fa, Fb, what)
    M, n_iter, var_floor, rho_max, min_count = _fit_args(n_components, n_iter, var_floor, rho_max, min_count, what)
    ev._need_gpu(what)
    d_la, d_lb, d_min = ev._upload_lens(h_a, h_b, np.minimum(h_a, h_b))
    if path is not None:
        path, d_plen = _i32_dev(path), _i32_dev(path_len)
    else:
        d_plen = d_min
    return _fit_device(speaker._f32(feat_src), speaker._f32(feat_tgt), d_la, d_lb, path, d_plen, M, n_iter, var_floor, rho_max,
                       min_count)


def _convert_device(model, table, cep, d_len, mixture, mlpg):
    """Static cepstra [B, F, n] on the device -> (converted statics, map result)."""
    M = model.w.shape[0]
    n = cep.shape[2]
    feat = speaker._features_launch(cep, d_len, None, True, False)
    r = _map_launch(feat, d_len, table, M, mixture, want_mmse=not mlpg)
    if mlpg:
        return _mlpg_launch(r.P, r.R, d_len).y, r
    return r.mmse[:, :, :n].contiguous(), r


def fit_wav(wav_src, lens_src, wav_tgt, lens_tgt, cfg_d, n_coef=24, n_realign=0, first_coef=1, wav_sr_src=None, wav_sr_tgt=None,
            res_type='kaiser_best', band=None, mixture='soft', n_components=32, n_iter=20, var_floor=1e-4, rho_max=0.99,
            min_count=1.0):
    """fit from B pairs of parallel recordings: the resampler (when a side's rate differs from cfg_d['sample_rate']), the
    front-end's mel, evaluation.mel_cepstra, the features, evaluation.dtw_batch(return_path=True) on the static cepstra and
    fit.  n_realign: that many times more, the DTW is run again between the CONVERTED source (convert_cepstra_batch with
    ``mixture``, MLPG) and the target, and the model is fitted again from its initialisation on the new paths (sprocket's
    loop).  wav [B, Lmax] float32; lens in samples at the side's own rate (None: the whole row).  Returns (JDGMM, trace) of
    the last fit."""
    import audio_lib
    what = 'mapping.fit_wav'
    if cfg_d is None:
        raise ValueError(' - ERROR, {}: cfg_d (the data-set configuration) is required'.format(what))
    audio_lib._res_params(res_type)
    a = ev._wav_side(wav_src, lens_src, cfg_d, wav_sr_src, 'wav_src')
    b = ev._wav_side(wav_tgt, lens_tgt, cfg_d, wav_sr_tgt, 'wav_tgt')
    if a['B'] != b['B']:
        raise ValueError(' - ERROR, {}: wav_src and wav_tgt must hold the same number of utterances'.format(what))
    n_coef, first_coef = int(n_coef), int(first_coef)
    ev.dct_rows(int(cfg_d['n_mels']), n_coef, first_coef)
    ev._check_pairs(a['B'], a['Fmax'], b['Fmax'], n_coef, True)
    band = ev._check_band(band)
    n_realign = speaker._check_count(n_realign, what + ': n_realign', 0, 100)
    mix = _check_mixture(mixture, what)
    M, n_iter, var_floor, rho_max, min_count = _fit_args(n_components, n_iter, var_floor, rho_max, min_count, what)
    ev._need_gpu(what)
    d_in_a, d_len_a, d_fa, d_in_b, d_len_b, d_fb, d_min = ev._upload_lens(a['h_in'], a['h'], a['n_frames'], b['h_in'], b['h'],
                                                                        b['n_frames'], np.minimum(a['n_frames'], b['n_frames']))
    ca = ev._cepstra_launch(ev._wav_mel(wav_src, a, d_in_a, d_len_a, cfg_d, res_type), n_coef, first_coef)
    cb = ev._cepstra_launch(ev._wav_mel(wav_tgt, b, d_in_b, d_len_b, cfg_d, res_type), n_coef, first_coef)
    fa, fb = speaker._features_launch(ca, d_fa, None, True, False), speaker._features_launch(cb, d_fb, None, True, False)
    r = ev._dtw_launch(ca, cb, d_fa, d_fb, 1.0, band, True)
    model, trace = _fit_device(fa, fb, d_fa, d_fb, r.path, r.path_len, M, n_iter, var_floor, rho_max, min_count)
    for _ in range(n_realign):
        conv, _ = _convert_device(model, _prepare_launch(model), ca, d_fa, mix, True)
        r = ev._dtw_launch(conv, cb, d_fa, d_fb, 1.0, band, True)
        model, trace = _fit_device(fa, fb, d_fa, d_fb, r.path, r.path_len, M, n_iter, var_floor, rho_max, min_count)
    return model, trace


def map_batch(model, feat, lens, mixture='soft'):
    """Conversion statistics of feat [B, F, D] (float32) under the model: P [B, F, D] the conditional precisions of the
    target's features summed over the posteriors of the source's marginal mixture, R [B, F, D] the precision-weighted
    conditional means, mmse [B, F, D] the frame-wise estimate sum gamma_m E_m, best [B, F] int32 the most likely component.
    mixture: 'soft' (every component, by its posterior) or 'best' (the most likely one alone).  Rows at or beyond an
    utterance's length are 0.  All on the device."""
    what = 'mapping.map_batch'
    B, F, D = speaker._check_feat(feat, what)
    M = _check_model(model, D, what)
    h = ev._check_lens(lens, B, F, what + ': lens')
    mix = _check_mixture(mixture, what)
    ev._need_gpu(what)
    d_len, = ev._upload_lens(h)
    model = _model_to_device(model)
    return _map_launch(speaker._f32(feat), d_len, _prepare_launch(model), M, mix)


def mlpg_batch(P, R, lens):
    """Maximum-likelihood parameter generation: P, R [B, F, 2 n] as map_batch returns them -> y [B, F, n], the static
    trajectories whose statics and deltas agree best with them, and flags [B] int32 (bit 0: a pivot of the banded solve was
    not positive and finite; the dimension it happened in holds R / P of the statics).  float64 on the device, rounded
    once."""
    what = 'mapping.mlpg_batch'
    B, F, D = speaker._check_feat(P, what + ': P')
    if tuple(getattr(R, 'shape', ())) != (B, F, D) or not speaker._is_f32(R):
        raise ValueError(' - ERROR, {}: R must be float32 [{}, {}, {}] like P'.format(what, B, F, D))
    _check_even(D, what)
    if F > MLPG_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: at most 2^20 frames'.format(what))
    h = ev._check_lens(lens, B, F, what + ': lens')
    ev._need_gpu(what)
    d_len, = ev._upload_lens(h)
    return _mlpg_launch(speaker._f32(P), speaker._f32(R), d_len)


def convert_cepstra_batch(model, cep, lens, mixture='soft', mlpg=True):
    """Static cepstra cep [B, F, n] (float32, evaluation.mel_cepstra) of the source converted under the model: the features
    (statics and their +-2 frame regression), map_batch's statistics and, with mlpg, the generated trajectory; without, the
    statics of the frame-wise estimate.  Returns [B, F, n] float32 on the device, zeros from an utterance's length on."""
    what = 'mapping.convert_cepstra_batch'
    if getattr(cep, 'ndim', 0) != 3 or min(cep.shape) < 1 or not speaker._is_f32(cep):
        raise ValueError(' - ERROR, {}: cep must be float32 [B, F, n]'.format(what))
    B, F, n = (int(v) for v in cep.shape)
    if n > MAX_COEF or B > 65535 or F > MLPG_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most 2^20 frames of at most {} coefficients'.format(what, MAX_COEF))
    M = _check_model(model, 2 * n, what)
    h = ev._check_lens(lens, B, F, what + ': lens')
    mix = _check_mixture(mixture, what)
    ev._need_gpu(what)
    d_len, = ev._upload_lens(h)
    model = _model_to_device(model)
    return _convert_device(model, _prepare_launch(model), speaker._f32(cep), d_len, mix, bool(mlpg))[0]


def _gain_args(cfg_d, n, first_coef, what):
    """(dct rows float32 [n, n_mels], i0, w, db_scale) on the host."""
    n_mels = int(cfg_d['n_mels'])
    if not 2 <= n_mels <= GAIN_MAX_MELS:
        raise ValueError(' - ERROR, {}: the gain takes 2 to {} mel bands (got {})'.format(what, GAIN_MAX_MELS, n_mels))
    dct = ev.dct_rows(n_mels, n, first_coef)
    i0, w = gain_tables(cfg_d)
    if len(i0) > GAIN_MAX_BINS:
        raise ValueError(' - ERROR, {}: at most {} bins'.format(what, GAIN_MAX_BINS))
    return dct, i0, w, db_scale(cfg_d)


def _gain_upload(i0, w):
    import torch
    return (torch.from_numpy(i0).pin_memory().to('cuda', non_blocking=True), torch.from_numpy(w).pin_memory().to('cuda', non_blocking=True))


def cepstra_gain_batch(cep_pred, cep_src, n_frames, cfg_d, alpha=1.0, max_boost_db=20.0, max_cut_db=30.0, first_coef=1):
    """The gain of the differential filter from converted and source static cepstra [B, F, n] (vc_cep_gain_f32): the
    cepstral difference back on the mel bands (the transpose of the DCT rows first_coef .. first_coef + n - 1), interpolated to
    the STFT bins by the front-end's own filterbank, scaled to dB, by alpha, clamped to [-max_cut_db, max_boost_db] and
    turned into an amplitude ratio.  n_frames: host integers, an int32 [B] device tensor or None (all F).  Returns
    [B, F, bins] float32 on the device, 0 in the rows at or beyond n_frames."""
    import torch
    import conversion
    what = 'mapping.cepstra_gain_batch'
    if cfg_d is None:
        raise ValueError(' - ERROR, {}: cfg_d (the data-set configuration) is required'.format(what))
    alpha, boost, cut = conversion._check_diff_args(alpha, max_boost_db, max_cut_db, what)
    if getattr(cep_pred, 'ndim', 0) != 3 or tuple(getattr(cep_src, 'shape', ())) != tuple(cep_pred.shape) or min(cep_pred.shape) < 1:
        raise ValueError(' - ERROR, {}: cep_pred and cep_src must be [B, F, n], the same shape'.format(what))
    if not (speaker._is_f32(cep_pred) and speaker._is_f32(cep_src)):
        raise ValueError(' - ERROR, {}: cep_pred and cep_src must be float32'.format(what))
    B, F, n = (int(v) for v in cep_pred.shape)
    dct, i0, w, scale = _gain_args(cfg_d, n, int(first_coef), what)
    if B > 65535 or F * len(i0) > 2 ** 30:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most 2^30 / bins frames'.format(what))
    if n_frames is not None and not (torch.is_tensor(n_frames) and n_frames.is_cuda):
        h = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > F:
            raise ValueError(' - ERROR, {}: n_frames must be {} integers in [0, {}]'.format(what, B, F))
    ev._need_gpu(what)
    d_nf = None if n_frames is None else conversion._i32_device(n_frames, (B,), what + ': n_frames')
    d_i0, d_w = _gain_upload(i0, w)
    return _gain_launch(speaker._f32(cep_pred), speaker._f32(cep_src), d_nf, ev._dct_device(int(cfg_d['n_mels']), n, int(first_coef)),
                        d_i0, d_w, alpha, scale, boost, cut)
