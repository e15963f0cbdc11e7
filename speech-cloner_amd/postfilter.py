"""Postfilters for converted spectra (include/vc_hip.h, "Postfilters"; csrc/vc_postfilter.hip): Toda's global-variance
filter and Takamichi's modulation-spectrum filter on trajectories x [B, maxF, C] float32 on the device.

  traj_stats_batch, gv_filter_batch, ms_stats_batch, ms_filter_batch     the four launches, one call each
  fit, model_from_stats, ms_coef, save, load                             the model: statistics of natural and generated spectra
  upload, apply_batch                                                    the chain of launches for one batch

A model is fitted once per target speaker: ``natural`` are the speaker's own spectra from the front-end
(audio_lib.calc_MFCC_input_batch), ``generated`` what the decoder predicts for training utterances
(conversion.convert_batch(vocode=False).stft_pred).  conversion.convert_postfilter_batch applies it between the stitch
and the vocoder.  The differential route is not wired up: hand apply_batch's output to conversion.diff_gain_batch as
``stft_pred`` to filter the source by a postfiltered envelope.

Nobody has listened to the result, and the repository carries no trained decoder: what is established is that the filters
compute their definition (tests/test_postfilter_gpu.py) and that the definition restores the statistics of a synthetic
over-smoothed corpus (tests/test_postfilter_cpu.py).  There is no CPU fallback."""
from collections import namedtuple

import numpy as np

N_BINS = 33                 # modulation bins of a 64-frame segment
MAX_BATCH, MAX_FRAMES, MAX_CHANNELS = 65535, 16384, 2049        # beyond: VC_ERR_UNSUPPORTED

Model = namedtuple('postfilter_model', 'gv_t mu_N sd_N mu_G sd_G usable')
Tables = namedtuple('postfilter_tables', 'coef gv_t k')


# ------------------------------------------------------------------------------------------ the four launches
def _inputs(what, x, n_frames):
    import torch
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if x.ndim != 3:
        raise ValueError(' - ERROR, {}: x must be [B, max_frames, C]'.format(what))
    x = x.to(device='cuda', dtype=torch.float32).contiguous()
    if n_frames is not None:
        if not torch.is_tensor(n_frames):
            n_frames = torch.from_numpy(np.asarray(n_frames, dtype=np.int32).reshape(-1))
        n_frames = n_frames.to(device='cuda', dtype=torch.int32).contiguous()
        if tuple(n_frames.shape) != (x.shape[0],):
            raise ValueError(' - ERROR, {}: n_frames must be [B]'.format(what))
    return x, n_frames


def _f32_device(t, shape, what):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    t = t.to(device='cuda', dtype=torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(' - ERROR, {} must be {}, got {}'.format(what, list(shape), list(t.shape)))
    return t


def traj_stats_batch(x, n_frames=None):
    """vc_traj_stats_f32: x [B, maxF, C] -> [B, C, 2] (mean, population variance over the first n_frames[b] frames)."""
    import torch
    import _vc
    x, n_frames = _inputs('traj_stats_batch', x, n_frames)
    B, F, C = x.shape
    out = torch.empty((B, C, 2), dtype=torch.float32, device=x.device)
    _vc.check(_vc.lib().vc_traj_stats_f32(_vc.ptr(x), _vc.ptr(n_frames), B, F, C, _vc.ptr(out), _vc.current_stream()))
    return out


def gv_filter_batch(x, n_frames, stats, gv_t, alpha=1.0, g_max=4.0):
    """vc_gv_filter_f32: every trajectory scaled about its mean towards the variance gv_t [C]; rows beyond n_frames are 0."""
    import torch
    import _vc
    x, n_frames = _inputs('gv_filter_batch', x, n_frames)
    B, F, C = x.shape
    stats, gv_t = _f32_device(stats, (B, C, 2), 'gv_filter_batch: stats'), _f32_device(gv_t, (C,), 'gv_filter_batch: gv_t')
    y = torch.empty_like(x)
    _vc.check(_vc.lib().vc_gv_filter_f32(_vc.ptr(x), _vc.ptr(n_frames), _vc.ptr(stats), _vc.ptr(gv_t), B, F, C, float(alpha),
                                         float(g_max), _vc.ptr(y), _vc.current_stream()))
    return y


def ms_stats_batch(x, n_frames, stats):
    """vc_ms_stats_f32: -> [B, C, 33, 3] (segments above the floor, sum and sum of squares of ln |X|^2) per modulation bin."""
    import torch
    import _vc
    x, n_frames = _inputs('ms_stats_batch', x, n_frames)
    B, F, C = x.shape
    stats = _f32_device(stats, (B, C, 2), 'ms_stats_batch: stats')
    out = torch.empty((B, C, N_BINS, 3), dtype=torch.float32, device=x.device)
    _vc.check(_vc.lib().vc_ms_stats_f32(_vc.ptr(x), _vc.ptr(n_frames), _vc.ptr(stats), B, F, C, _vc.ptr(out), _vc.current_stream()))
    return out


def ms_filter_batch(x, n_frames, stats, coef, lo, hi):
    """vc_ms_filter_f32: coef [C, 33, 2] = (a, b); lo <= 0 <= hi clamp the natural-log amplitude exponent a s + b."""
    import torch
    import _vc
    x, n_frames = _inputs('ms_filter_batch', x, n_frames)
    B, F, C = x.shape
    stats, coef = _f32_device(stats, (B, C, 2), 'ms_filter_batch: stats'), _f32_device(coef, (C, N_BINS, 2), 'ms_filter_batch: coef')
    y = torch.empty_like(x)
    _vc.check(_vc.lib().vc_ms_filter_f32(_vc.ptr(x), _vc.ptr(n_frames), _vc.ptr(stats), _vc.ptr(coef), B, F, C, float(lo), float(hi),
                                         _vc.ptr(y), _vc.current_stream()))
    return y


# ------------------------------------------------------------------------------------------ the model (host, float64)
def _combine(ms_list):
    tot = None
    for ms in ms_list:
        ms = np.asarray(ms.cpu() if hasattr(ms, 'cpu') else ms, dtype=np.float64)
        if ms.ndim != 4 or ms.shape[2:] != (N_BINS, 3):
            raise ValueError(' - ERROR, postfilter: modulation statistics must be [B, C, 33, 3]')
        tot = ms.sum(0) if tot is None else tot + ms.sum(0)
    cnt, s1, s2 = tot[:, :, 0], tot[:, :, 1], tot[:, :, 2]
    safe = np.maximum(cnt, 1.0)
    mu = s1 / safe
    return cnt, mu, np.sqrt(np.maximum(s2 / safe - mu * mu, 0.0))


def model_from_stats(natural_stats, natural_ms, generated_ms):
    """The model from what the launches return.  natural_stats: a list of (stats [B, C, 2], n_frames [B]) of natural batches;
    natural_ms, generated_ms: lists of [B, C, 33, 3].  gv_t is the mean of the natural per-utterance variances (empty
    utterances left out); mu and sd are the mean and the population deviation of ln |X|^2 over all segments, from the
    counts and sums in float64.  An entry with fewer than 2 segments on either side, or with no spread, is unusable."""
    var, k = 0.0, 0
    for st, n in natural_stats:
        st = np.asarray(st.cpu() if hasattr(st, 'cpu') else st, dtype=np.float64)
        n = np.asarray(n.cpu() if hasattr(n, 'cpu') else n).reshape(-1)
        var, k = var + st[n > 0, :, 1].sum(0), k + int((n > 0).sum())
    if k == 0:
        raise ValueError(' - ERROR, postfilter: no natural utterance to fit on')
    cN, mu_N, sd_N = _combine(natural_ms)
    cG, mu_G, sd_G = _combine(generated_ms)
    if mu_N.shape != mu_G.shape or mu_N.shape[0] != np.shape(var)[0]:
        raise ValueError(' - ERROR, postfilter: natural and generated statistics differ in their channel count')
    usable = (cN >= 2) & (cG >= 2) & (sd_N > 0) & (sd_G > 0)
    return Model(var / k, mu_N, sd_N, mu_G, sd_G, usable)


def fit(natural, generated):
    """natural, generated: lists of (x [B, maxF, C], n_frames [B] or None) batches -> Model.  Runs vc_traj_stats_f32 and
    vc_ms_stats_f32 on every batch and combines the results on the host in float64."""
    nat_st, nat_ms, gen_ms = [], [], []
    for x, n in natural:
        st = traj_stats_batch(x, n)
        nat_st.append((st, np.full((st.shape[0],), int(x.shape[1])) if n is None else n))
        nat_ms.append(ms_stats_batch(x, n, st))
    for x, n in generated:
        gen_ms.append(ms_stats_batch(x, n, traj_stats_batch(x, n)))
    if not nat_ms or not gen_ms:
        raise ValueError(' - ERROR, postfilter.fit: needs at least one natural and one generated batch')
    return model_from_stats(nat_st, nat_ms, gen_ms)


def ms_coef(model, k=0.85):
    """[C, 33, 2] float32 (a, b): the exponent a s + b moves a bin's ln |X|^2 = s a fraction k of the way from the generated
    to the natural distribution, s -> (sd_N / sd_G)(s - mu_G) + mu_N, halved because it scales amplitudes:
    a = 0.5 k (sd_N / sd_G - 1), b = 0.5 k (mu_N - (sd_N / sd_G) mu_G).  Unusable entries and bin 0 are 0."""
    k = float(k)
    if not 0.0 <= k <= 1.0:
        raise ValueError(' - ERROR, postfilter.ms_coef: k must lie in [0, 1], got {!r}'.format(k))
    ok = np.asarray(model.usable, dtype=bool).copy()
    ok[:, 0] = False
    r = np.where(ok, model.sd_N / np.where(ok, model.sd_G, 1.0), 1.0)
    a = np.where(ok, 0.5 * k * (r - 1.0), 0.0)
    b = np.where(ok, 0.5 * k * (model.mu_N - r * model.mu_G), 0.0)
    return np.stack([a, b], -1).astype(np.float32)


def save(path, model):
    np.savez(path, **{f: np.asarray(getattr(model, f)) for f in Model._fields})


def load(path):
    with np.load(path) as z:
        return Model(*(z[f] for f in Model._fields))


# ------------------------------------------------------------------------------------------ applying a model
def upload(model, k=0.85):
    """The model's device tables for apply_batch (coef [C, 33, 2] at strength k, gv_t [C]): make them once per model."""
    import torch
    coef = torch.from_numpy(ms_coef(model, k)).to('cuda')
    return Tables(coef, torch.from_numpy(np.asarray(model.gv_t, dtype=np.float32)).to('cuda'), float(k))


_MODES = ('ms', 'gv', 'ms+gv')


def check_apply_args(mode, k, alpha, max_db, g_max, what='apply_batch'):
    if mode not in _MODES:
        raise ValueError(" - ERROR, {}: mode must be 'ms', 'gv' or 'ms+gv', got {!r}".format(what, mode))
    for name, v, lo, hi in (('k', k, 0.0, 1.0), ('alpha', alpha, 0.0, 1.0), ('max_db', max_db, 0.0, 200.0), ('g_max', g_max, 1.0, 1e6)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:
            raise ValueError(' - ERROR, {}: {} must be a number in [{}, {}], got {!r}'.format(what, name, lo, hi, v))


def apply_batch(x, n_frames, model, mode='ms', k=0.85, alpha=1.0, max_db=20.0, g_max=4.0):
    """x [B, maxF, C] float32 (stft_pred, mel_pred or any dB-linear feature), n_frames int32 [B] on the device (or host ints,
    or None) -> the filtered trajectories, zero from n_frames on.  model: a Model or upload()'s tables (then ``k`` is the
    tables' own).  mode 'ms': statistics, then the modulation-spectrum filter at strength k with the gain of a bin kept
    within +-max_db; 'gv': statistics, then the global-variance filter at strength alpha with the gain within
    [1 / g_max, g_max]; 'ms+gv': the first, then the second on statistics recomputed from the first's output.  Launches
    only: nothing is copied to the host."""
    check_apply_args(mode, k, alpha, max_db, g_max)
    t = model if isinstance(model, Tables) else upload(model, k)
    x, n_frames = _inputs('apply_batch', x, n_frames)
    if x.shape[2] != t.gv_t.shape[0]:
        raise ValueError(' - ERROR, apply_batch: the model has {} channels, x has {}'.format(t.gv_t.shape[0], x.shape[2]))
    y = x
    if mode in ('ms', 'ms+gv'):
        hi = float(max_db) * np.log(10.0) / 20.0
        y = ms_filter_batch(y, n_frames, traj_stats_batch(y, n_frames), t.coef, -hi, hi)
    if mode in ('gv', 'ms+gv'):
        y = gv_filter_batch(y, n_frames, traj_stats_batch(y, n_frames), t.gv_t, alpha, g_max)
    return y
