"""Speaker similarity on the MI355X: does a conversion sound like the target speaker, and no longer like the source?

The text-independent answer that needs no parallel sentence and no pretrained model (Reynolds, Quatieri and Dunn 2000): a
diagonal-covariance Gaussian mixture fitted on the cepstral features of many speakers, the universal background model
(UBM); the same mixture with its means MAP-adapted to each speaker; and the mean per-frame log-likelihood ratio (LLR) of an
utterance between the claimed speaker's model and the UBM.

  features_batch(mel, lens, n_coef, first_coef, deltas, cmn, mask)          -> feat [B, F, D]: cepstra, deltas, mean removed
  gmm_fit(feat, lens, n_components, n_iter, mask, var_floor, min_count)     -> (GMM(weights, means, variances), trace [n_iter])
  gmm_adapt_batch(ubm, feat, lens, groups, n_groups, relevance, mask)       -> means [S, M, D], one model per group
  gmm_score_batch(ubm, spk_means, feat, lens, model_index, mask)            -> (llr, ll_spk, ll_ubm, n_frames), [B] each
  speaker_wav_batch(ubm, spk_means, wav, lens, model_index, cfg_d, ...)     resampler, front-end and the two above in one

Definitions: include/vc_hip.h, "Speaker"; DESIGN.md section 18.  Lengths, groups and model indices are host integers.
Every check is made on the host before the first launch; after that nothing is copied to the host and the host waits for
nothing.  All arithmetic runs in csrc/vc_gmm.hip; the E-step never stores the [frames, components] posteriors.  There is
no CPU path.
"""
from collections import namedtuple

import numpy as np

import _vc
import evaluation as ev

MAX_COMPONENTS = 256
MAX_DIM = 64
MAX_MODELS = 4096
MAX_ELEMS = 2 ** 30             # frames * D of one utterance
GMM_TILE_FRAMES = 32            # vc_gmm_tile_frames(): frames per workgroup of the log-likelihood and E-step launches

GMM = namedtuple('GMM', 'weights means variances')
_SCORE = namedtuple('speaker_score', 'llr ll_spk ll_ubm n_frames')
_WAV = namedtuple('speaker_wav', 'llr ll_spk ll_ubm n_frames feat mask')
_STATS = namedtuple('gmm_stats', 'N S1 S2 L')


# ------------------------------------------------------------------------------------------------------------- host checks
def _is_f32(t):
    return str(getattr(t, 'dtype', None)) in ('torch.float32', 'float32')


def _check_feat(feat, what):
    if getattr(feat, 'ndim', 0) != 3 or min(feat.shape) < 1:
        raise ValueError(' - ERROR, {}: feat must be [B, F, D]'.format(what))
    if not _is_f32(feat):
        raise ValueError(' - ERROR, {}: feat must be float32, got {}'.format(what, getattr(feat, 'dtype', type(feat))))
    B, F, D = (int(v) for v in feat.shape)
    if D > MAX_DIM:
        raise ValueError(' - ERROR, {}: feat holds at most {} columns (got D = {})'.format(what, MAX_DIM, D))
    if B > 65535 or F * D > MAX_ELEMS:
        raise ValueError(' - ERROR, {}: feat holds at most 65535 utterances of at most 2^30 / D frames (got {} of {}, D = {})'
                         .format(what, B, F, D))
    return B, F, D


def _check_gmm(ubm, D, what):
    if not (isinstance(ubm, tuple) and len(ubm) == 3):
        raise ValueError(' - ERROR, {}: ubm must be a GMM(weights, means, variances)'.format(what))
    w, mu, var = ubm
    for t, name in ((w, 'weights'), (mu, 'means'), (var, 'variances')):
        if not _is_f32(t):
            raise ValueError(' - ERROR, {}: ubm.{} must be float32'.format(what, name))
    M = int(w.shape[0]) if getattr(w, 'ndim', 0) == 1 else 0
    if not 1 <= M <= MAX_COMPONENTS:
        raise ValueError(' - ERROR, {}: ubm.weights must be [M] with 1 <= M <= {}'.format(what, MAX_COMPONENTS))
    if tuple(mu.shape) != (M, D) or tuple(var.shape) != (M, D):
        raise ValueError(' - ERROR, {}: ubm.means and ubm.variances must be [M, D] = [{}, {}] like feat (got {} and {})'
                         .format(what, M, D, tuple(mu.shape), tuple(var.shape)))
    return M


def _check_index(idx, B, lo, hi, what):
    h = np.asarray(idx)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < lo or h.max() >= hi:
        raise ValueError(' - ERROR, {} must be {} integers in [{}, {})'.format(what, B, lo, hi))
    return h.astype(np.int64)


def _check_pos(v, what, lo=0.0, strict=False):
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float('nan')
    if not (np.isfinite(f) and (f > lo if strict else f >= lo)):
        raise ValueError(' - ERROR, {} must be finite and {} {}, got {!r}'.format(what, '>' if strict else '>=', lo, v))
    return f


def _check_count(v, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(' - ERROR, {} must be an integer in [{}, {}], got {!r}'.format(what, lo, hi, v))
    return int(v)


def _f32(t):
    import torch
    return ev._to_device(t, torch.float32)


# ---------------------------------------------------------------------------------------------------------------- launches
def _features_launch(cep, d_len, mask, deltas, cmn):
    """cep: cuda float32 [B, F, n_coef]; mask: cuda uint8 [B, F] or None.  No host check in here."""
    import torch
    B, F, n_coef = cep.shape
    out = torch.empty((B, F, n_coef * (2 if deltas else 1)), dtype=torch.float32, device=cep.device)
    _vc.check(_vc.lib().vc_spk_features_f32(_vc.ptr(cep), _vc.ptr(d_len), _vc.ptr(mask), B, F, n_coef, int(deltas), int(cmn), _vc.ptr(out),
                                            _vc.current_stream()))
    return out


def _prepare_launch(w, means, var):
    """w [M], means [S, M, D], var [M, D] -> the table of vc_gmm_prepare_f32."""
    import torch
    S, M, D = means.shape
    table = torch.empty((S + 1) * M * D + M, dtype=torch.float32, device=means.device)
    _vc.check(_vc.lib().vc_gmm_prepare_f32(_vc.ptr(w), _vc.ptr(means), _vc.ptr(var), S, M, D, _vc.ptr(table), _vc.current_stream()))
    return table


def _loglik_launch(feat, d_len, table, S, M, d_model, d_model_b=None):
    import torch
    B, F, D = feat.shape
    ll = torch.empty((B, F), dtype=torch.float32, device=feat.device)
    ll_b = torch.empty_like(ll) if d_model_b is not None else None
    _vc.check(_vc.lib().vc_gmm_loglik_f32(_vc.ptr(feat), _vc.ptr(d_len), B, F, D, _vc.ptr(table), S, M, _vc.ptr(d_model), _vc.ptr(ll),
                                          _vc.ptr(d_model_b), _vc.ptr(ll_b), _vc.current_stream()))
    return ll, ll_b


def _score_launch(ll_a, ll_b, d_len, mask):
    import torch
    B, F = ll_a.shape
    n = torch.empty((B,), dtype=torch.int32, device=ll_a.device)
    v = torch.empty((B, 3), dtype=torch.float32, device=ll_a.device)
    _vc.check(_vc.lib().vc_gmm_score_f32(_vc.ptr(ll_a), _vc.ptr(ll_b), _vc.ptr(d_len), _vc.ptr(mask), B, F, _vc.ptr(n), _vc.ptr(v),
                                         _vc.current_stream()))
    return _SCORE(v[:, 2], v[:, 0], v[:, 1], n)


def workspace_bytes(n_groups, M, D):
    """vc_gmm_workspace_bytes: host arithmetic."""
    return int(_vc.lib().vc_gmm_workspace_bytes(int(n_groups), int(M), int(D)))


def _accumulate_launch(feat, ll, d_len, mask, d_group, table, S, M, n_groups, model=0, ws=None):
    import torch
    B, F, D = feat.shape
    dev = feat.device
    st = _STATS(torch.empty((n_groups, M), dtype=torch.float64, device=dev), torch.empty((n_groups, M, D), dtype=torch.float64, device=dev),
                torch.empty((n_groups, M, D), dtype=torch.float64, device=dev), torch.empty((n_groups,), dtype=torch.float64, device=dev))
    if ws is None:
        need = workspace_bytes(n_groups, M, D)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    _vc.check(_vc.lib().vc_gmm_accumulate_f32(_vc.ptr(feat), _vc.ptr(ll), _vc.ptr(d_len), _vc.ptr(mask), _vc.ptr(d_group), B, F, D,
                                              _vc.ptr(table), S, M, model, n_groups, _vc.ptr(st.N), _vc.ptr(st.S1), _vc.ptr(st.S2),
                                              _vc.ptr(st.L), _vc.ptr(ws), 0 if ws is None else ws.numel(), _vc.current_stream()))
    return st


def _update_em_launch(st, mu, var, var_floor, min_count):
    import torch
    M, D = mu.shape
    w_out = torch.empty((M,), dtype=torch.float32, device=mu.device)
    mu_out, var_out = torch.empty_like(mu), torch.empty_like(var)
    _vc.check(_vc.lib().vc_gmm_update_f32(0, _vc.ptr(st.N), _vc.ptr(st.S1), _vc.ptr(st.S2), 1, M, D, _vc.ptr(mu), _vc.ptr(var),
                                          _vc.ptr(var_floor), float(min_count), 0.0, _vc.ptr(w_out), _vc.ptr(mu_out), _vc.ptr(var_out),
                                          _vc.current_stream()))
    return w_out, mu_out, var_out


def _update_map_launch(st, mu_ubm, relevance):
    import torch
    G, M, D = st.S1.shape
    out = torch.empty((G, M, D), dtype=torch.float32, device=mu_ubm.device)
    _vc.check(_vc.lib().vc_gmm_update_f32(1, _vc.ptr(st.N), _vc.ptr(st.S1), None, G, M, D, _vc.ptr(mu_ubm), None, None, 0.0,
                                          float(relevance), None, _vc.ptr(out), None, _vc.current_stream()))
    return out


def _gmm_to_device(ubm):
    return GMM(*(_f32(t) for t in ubm))


# ------------------------------------------------------------------------------------------------------------------ public
def features_batch(mel, lens, n_coef=24, first_coef=1, deltas=True, cmn=True, mask=None):
    """Speaker features of B utterances: the mel cepstra c[first_coef : first_coef + n_coef] (evaluation.mel_cepstra), with
    deltas their regression over +-2 frames, with cmn the mean over the kept frames removed.  mel [B, F, n_mels] as
    convert_batch returns it (float32 or bfloat16); lens: host integers in [1, F]; mask: uint8 or bool [B, F], 1 = the frame
    counts towards the mean (every frame is still written).  Returns feat [B, F, D], D = n_coef * (1 + deltas), float32 on
    the device, zeros from an utterance's length on."""
    B, F, n_mels = ev._check_mel(mel, 'features_batch: mel')
    n_coef, first_coef = int(n_coef), int(first_coef)
    ev.dct_rows(n_mels, n_coef, first_coef)
    D = n_coef * (2 if deltas else 1)
    if B > 65535 or F * D > MAX_ELEMS:
        raise ValueError(' - ERROR, features_batch: at most 65535 utterances of at most 2^30 / D frames (got {} of {}, D = {})'.format(B, F, D))
    h = ev._check_lens(lens, B, F, 'features_batch: lens')
    if mask is not None:
        _check_mask(mask, B, F, 'features_batch: mask')
    ev._need_gpu('features_batch')
    d_len, = ev._upload_lens(h)
    cep = ev._cepstra_launch(ev._to_device(mel), n_coef, first_coef)
    return _features_launch(cep, d_len, _mask_dev(mask), bool(deltas), bool(cmn))


def _check_mask(mask, B, F, what):
    import torch
    ok = (torch.uint8, torch.bool) if torch.is_tensor(mask) else (np.dtype(np.uint8), np.dtype(np.bool_))
    if getattr(mask, 'ndim', 0) != 2 or getattr(mask, 'dtype', None) not in ok:
        raise ValueError(' - ERROR, {} must be a uint8 or bool array [B, F], got {} {}'.format(what, getattr(mask, 'dtype', type(mask)),
                                                                                              tuple(getattr(mask, 'shape', ()))))
    if tuple(int(v) for v in mask.shape) != (B, F):
        raise ValueError(' - ERROR, {} must be [{}, {}] like feat, got {}'.format(what, B, F, tuple(mask.shape)))


def _mask_dev(mask):
    return None if mask is None else ev._mask_to_device(mask, 0, 0)


def gmm_fit(feat, lens, n_components=64, n_iter=10, mask=None, var_floor=0.01, min_count=1.0):
    """EM for a diagonal-covariance mixture of n_components on the kept frames of feat [B, F, D] (float32).

    Initialisation is deterministic: the means are the rows at positions floor((m + 1/2) n / M) of the concatenation of all
    n frames below lens, the variances the global variance of the kept frames (one E-step with a single component), the
    weights uniform.  var_floor: the floor of every variance as a fraction of that global variance per dimension;
    min_count: a component that gathers fewer frames keeps its mean and variance.  Every iteration is vc_gmm_prepare_f32,
    vc_gmm_loglik_f32, vc_gmm_accumulate_f32, vc_gmm_update_f32.  Returns (GMM(weights [M], means [M, D], variances [M, D]),
    trace [n_iter] float64): trace[i] is the mean log-likelihood per kept frame BEFORE update i.  All on the device."""
    import torch
    B, F, D = _check_feat(feat, 'gmm_fit')
    h = ev._check_lens(lens, B, F, 'gmm_fit: lens')
    M = _check_count(n_components, 'gmm_fit: n_components', 1, MAX_COMPONENTS)
    n_iter = _check_count(n_iter, 'gmm_fit: n_iter', 1, 10 ** 6)
    var_floor = _check_pos(var_floor, 'gmm_fit: var_floor', 0.0, strict=True)
    min_count = _check_pos(min_count, 'gmm_fit: min_count')
    if mask is not None:
        _check_mask(mask, B, F, 'gmm_fit: mask')
    n = int(h.sum())
    pos = ((2 * np.arange(M, dtype=np.int64) + 1) * n) // (2 * M)
    ends = np.cumsum(h)
    b = np.searchsorted(ends, pos, side='right')
    rows = b * F + (pos - (ends[b] - h[b]))
    ev._need_gpu('gmm_fit')
    lib, dev = _vc.lib(), 'cuda'
    d_len, = ev._upload_lens(h)
    d_rows = torch.from_numpy(rows).pin_memory().to(dev, non_blocking=True)
    feat, mask = _f32(feat), _mask_dev(mask)
    zeros = torch.zeros((B,), dtype=torch.int32, device=dev)
    need = max(workspace_bytes(1, M, D), workspace_bytes(1, 1, D))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    # the global variance: one component, mean 0, variance 1 (gamma = 1 exactly, so N is the count of kept frames)
    one = torch.ones((1 + D,), dtype=torch.float32, device=dev)
    mu0 = torch.zeros((1, D), dtype=torch.float32, device=dev)
    tab = _prepare_launch(one[:1], mu0[None], one[1:].view(1, D))
    st = _accumulate_launch(feat, _loglik_launch(feat, d_len, tab, 1, 1, zeros)[0], d_len, mask, zeros, tab, 1, 1, 1, ws=ws)
    n_kept = st.N[0, 0]
    gvar = _update_em_launch(st, mu0, one[1:].view(1, D), mu0[0], 0.0)[2]
    floor = (gvar[0] * var_floor).contiguous()
    mu = torch.empty((M, D), dtype=torch.float32, device=dev)
    _vc.check(lib.vc_gather_rows(_vc.ptr(feat), _vc.ptr(d_rows), None, M, D * 4, _vc.ptr(mu), _vc.current_stream()))
    var = gvar.expand(M, D).contiguous()
    w = torch.full((M,), 1.0 / M, dtype=torch.float32, device=dev)
    trace = torch.empty((n_iter,), dtype=torch.float64, device=dev)
    for i in range(n_iter):
        tab = _prepare_launch(w, mu[None], var)
        st = _accumulate_launch(feat, _loglik_launch(feat, d_len, tab, 1, M, zeros)[0], d_len, mask, zeros, tab, 1, M, 1, ws=ws)
        trace[i] = st.L[0] / n_kept
        w, mu, var = _update_em_launch(st, mu, var, floor, min_count)
    return GMM(w, mu, var), trace


def gmm_adapt_batch(ubm, feat, lens, groups, n_groups, relevance=16.0, mask=None):
    """MAP adaptation of the UBM's means to n_groups speakers in one pass: groups [B] names the speaker of every utterance
    (host integers in [0, n_groups), -1 = leave the utterance out).  alpha = N / (N + relevance) per component and
    speaker; a component a speaker never visits, and a speaker without utterances, keep the UBM's means bit for bit.
    Returns means [n_groups, M, D] float32 on the device; weights and variances stay the UBM's."""
    B, F, D = _check_feat(feat, 'gmm_adapt_batch')
    M = _check_gmm(ubm, D, 'gmm_adapt_batch')
    h = ev._check_lens(lens, B, F, 'gmm_adapt_batch: lens')
    G = _check_count(n_groups, 'gmm_adapt_batch: n_groups', 1, MAX_MODELS)
    hg = _check_index(groups, B, -1, G, 'gmm_adapt_batch: groups')
    relevance = _check_pos(relevance, 'gmm_adapt_batch: relevance')
    if mask is not None:
        _check_mask(mask, B, F, 'gmm_adapt_batch: mask')
    ev._need_gpu('gmm_adapt_batch')
    import torch
    d_len, d_group = ev._upload_lens(h, hg)
    feat, mask, ubm = _f32(feat), _mask_dev(mask), _gmm_to_device(ubm)
    tab = _prepare_launch(ubm.weights, ubm.means[None], ubm.variances)
    zeros = torch.zeros((B,), dtype=torch.int32, device=feat.device)
    ll = _loglik_launch(feat, d_len, tab, 1, M, zeros)[0]
    return _update_map_launch(_accumulate_launch(feat, ll, d_len, mask, d_group, tab, 1, M, G), ubm.means, relevance)


def _score_checks(ubm, spk_means, B, D, model_index, what):
    M = _check_gmm(ubm, D, what)
    if getattr(spk_means, 'ndim', 0) != 3 or tuple(spk_means.shape[1:]) != (M, D) or not 1 <= int(spk_means.shape[0]) <= MAX_MODELS:
        raise ValueError(' - ERROR, {}: spk_means must be [S, M, D] = [1 .. {}, {}, {}], got {}'
                         .format(what, MAX_MODELS, M, D, tuple(getattr(spk_means, 'shape', ()))))
    if not _is_f32(spk_means):
        raise ValueError(' - ERROR, {}: spk_means must be float32, got {}'.format(what, spk_means.dtype))
    return M, _check_index(model_index, B, 0, int(spk_means.shape[0]), what + ': model_index')


def _score_chain(ubm, spk_means, feat, d_len, d_model, mask):
    """Model 0 of the table is the UBM, model s + 1 speaker s; d_model holds s + 1."""
    import torch
    S, M, D = spk_means.shape
    tab = _prepare_launch(ubm.weights, torch.cat([ubm.means[None], spk_means]), ubm.variances)
    ll_a, ll_b = _loglik_launch(feat, d_len, tab, S + 1, M, d_model, torch.zeros_like(d_model))
    return _score_launch(ll_a, ll_b, d_len, mask)


def gmm_score_batch(ubm, spk_means, feat, lens, model_index, mask=None):
    """The mean per-frame log-likelihood ratio of B utterances between speaker model_index[b] (spk_means [S, M, D], as
    gmm_adapt_batch returns them) and the UBM, over the kept frames.  Returns a namedtuple of [B] device tensors: llr =
    ll_spk - ll_ubm, ll_spk, ll_ubm (float32) and n_frames (int32); an utterance without a kept frame has n_frames = 0 and NaN
    figures.  An utterance's figures do not depend on the batch it is scored in."""
    B, F, D = _check_feat(feat, 'gmm_score_batch')
    M, hm = _score_checks(ubm, spk_means, B, D, model_index, 'gmm_score_batch')
    h = ev._check_lens(lens, B, F, 'gmm_score_batch: lens')
    if mask is not None:
        _check_mask(mask, B, F, 'gmm_score_batch: mask')
    ev._need_gpu('gmm_score_batch')
    d_len, d_model = ev._upload_lens(h, hm + 1)
    return _score_chain(_gmm_to_device(ubm), _f32(spk_means), _f32(feat), d_len, d_model, _mask_dev(mask))


def speaker_wav_batch(ubm, spk_means, wav, lens, model_index, cfg_d, wav_sr=None, res_type='kaiser_best', mask=None, n_coef=24,
                      first_coef=1, deltas=True, cmn=True, top_db=40.0, max_gap=20, min_run=0, frame_length=512, fmin=60.0,
                      fmax=400.0, threshold=0.15):
    """"How much does this waveform sound like speaker s" in one call: the resampler (when wav_sr differs from
    cfg_d['sample_rate']), the front-end's mel (the path evaluation.mcd_wav_batch takes), features_batch and
    gmm_score_batch.  wav [B, Lmax] float32, lens host integers in samples at the waveform's own rate (None = the whole
    row).  mask: None; 'energy', 'voiced' or 'energy+voiced': a speech-activity mask made as evaluation.score_wav_batch
    makes it (top_db, max_gap, min_run; the tracker's frame_length, fmin, fmax, threshold), the front-end's amplitude
    normalisation then taken over the speech samples; or a uint8 / bool array [B, 1 + Lmax // hop] taken as given.  The
    mask selects the frames of the cepstral mean and of the score.  Returns gmm_score_batch's four fields, feat and mask."""
    import audio_lib
    if cfg_d is None:
        raise ValueError(' - ERROR, speaker_wav_batch: cfg_d (the data-set configuration) is required')
    audio_lib._res_params(res_type)
    side = ev._wav_side(wav, lens, cfg_d, wav_sr, 'wav')
    B, Fmax = side['B'], side['Fmax']
    n_coef, first_coef = int(n_coef), int(first_coef)
    ev.dct_rows(int(cfg_d['n_mels']), n_coef, first_coef)
    D = n_coef * (2 if deltas else 1)
    if B > 65535 or Fmax * D > MAX_ELEMS:
        raise ValueError(' - ERROR, speaker_wav_batch: at most 65535 utterances of at most 2^30 / D frames')
    M, hm = _score_checks(ubm, spk_means, B, D, model_index, 'speaker_wav_batch')
    act = args = None
    if isinstance(mask, str):
        act = ev._activity_args(mask, top_db, max_gap, min_run, 'speaker_wav_batch')
        ev._check_energy(cfg_d['hop_length'], cfg_d['win_length'], Fmax, 'speaker_wav_batch')
        if act[0] & 2:
            args = ev._f0_args(cfg_d['sample_rate'], cfg_d['hop_length'], frame_length, fmin, fmax, threshold, 'speaker_wav_batch')
    elif mask is not None:
        _check_mask(mask, B, Fmax, 'speaker_wav_batch: mask')
    ev._need_gpu('speaker_wav_batch')
    d_in, d_len, d_frames, d_model = ev._upload_lens(side['h_in'], side['h'], side['n_frames'], hm + 1)
    x = ev._wav_at_rate(wav, side, d_in, cfg_d, res_type)
    if act is not None:
        x = x.contiguous()
        m = ev._wav_mask(x, d_len, d_frames, cfg_d, act, ev._f0_launch(x, d_len, args)[0] if args else None)
        mel = ev._speech_mel(x, d_len, m, ev._compact_launch(m, d_frames).n_active, cfg_d)
    else:
        m = _mask_dev(mask)
        mel = ev._mel_launch(x, d_len, cfg_d)
    feat = _features_launch(ev._cepstra_launch(mel, n_coef, first_coef), d_frames, m, bool(deltas), bool(cmn))
    r = _score_chain(_gmm_to_device(ubm), _f32(spk_means), feat, d_frames, d_model, m)
    return _WAV(r.llr, r.ll_spk, r.ll_ubm, r.n_frames, feat, m)
