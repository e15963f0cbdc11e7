"""Noise suppression on the device (include/vc_hip.h, "Noise suppression"): stationary noise taken out of a waveform before it
is analysed or converted.  Three launches and the overlap-add:

    power   P = |stft(x)|^2                                     audio_lib.stft_power_batch   (vc_stft_power_f32)
    gain    noise tracker + suppression rule, one scan in time  noise_gain_batch             (vc_noise_gain_f32)
    filter  y = istft(G * stft(x))                              audio_lib.stft_filter_batch  (vc_stft_filter_f32)

The tracker is Gerkmann & Hendriks' speech-presence-probability estimator (2012), the rule Ephraim & Malah's log-MMSE
amplitude estimator (or the Wiener gain) on the decision-directed a-priori SNR with Cappe's lower limit.  The defaults are
the literature's, carried to this project's 5 ms hop (``smoothing``); nobody has listened to anything they produce.
tests/denoise_ref.py restates both new launches in numpy.  There is no CPU fallback: without a GPU every call raises."""
import collections
import math

import numpy as np

import _vc

RULES = {'wiener': 0, 'logmmse': 1}
_DENOISE_NT = collections.namedtuple('denoise', 'y gain noise n_frames')
GAIN_KEYS = ('rule', 'noise0', 'n_init', 'a_spp', 'a_noise', 'a_dd', 'xi_h1_db', 'xi_min_db', 'floor_db', 'gamma_max', 'return_noise')


def smoothing(hop_length, sr, tau_spp_ms=151.9, tau_noise_ms=71.7):
    """(a_spp, a_noise) = exp(-hop / tau) for this hop.  The defaults are the time constants behind Gerkmann & Hendriks'
    0.9 and 0.8 at their 16 ms hop: a recursion run every 5 ms with the constants of a 16 ms hop forgets three times as fast
    and follows voiced speech instead of the noise."""
    for v, name in ((hop_length, 'hop_length'), (sr, 'sr'), (tau_spp_ms, 'tau_spp_ms'), (tau_noise_ms, 'tau_noise_ms')):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v <= 0:
            raise ValueError(' - ERROR, smoothing: {} must be a positive number, got {!r}'.format(name, v))
    hop_ms = 1000.0 * float(hop_length) / float(sr)
    return math.exp(-hop_ms / float(tau_spp_ms)), math.exp(-hop_ms / float(tau_noise_ms))


def _number(v, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(' - ERROR, {}: {} must be a finite number, got {!r}'.format(what, name, v))
    return float(v)


def gain_cfg(what, rule='logmmse', n_init=8, a_spp=None, a_noise=None, a_dd=0.98, xi_h1_db=15, xi_min_db=-25, floor_db=20,
             gamma_max=1000.0, hop_length=80, sr=16000):
    """The checked vc_denoise_cfg of a noise_gain_batch call (ValueError otherwise; no GPU).  a_spp / a_noise None: those of
    ``smoothing(hop_length, sr)``."""
    if not isinstance(rule, str) or rule not in RULES:
        raise ValueError(" - ERROR, {}: rule must be 'logmmse' or 'wiener', got {!r}".format(what, rule))
    if isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or not 1 <= n_init < 2 ** 31:
        raise ValueError(' - ERROR, {}: n_init must be an integer >= 1, got {!r}'.format(what, n_init))
    d_spp, d_noise = smoothing(hop_length, sr)
    a_spp = d_spp if a_spp is None else _number(a_spp, what, 'a_spp')
    a_noise = d_noise if a_noise is None else _number(a_noise, what, 'a_noise')
    a_dd = _number(a_dd, what, 'a_dd')
    if not (0.0 <= a_spp <= 1.0 and 0.0 <= a_dd <= 1.0):
        raise ValueError(' - ERROR, {}: a_spp and a_dd must be in [0, 1], got {!r}, {!r}'.format(what, a_spp, a_dd))
    if not 0.0 < a_noise <= 1.0:
        raise ValueError(' - ERROR, {}: a_noise must be in (0, 1], got {!r}'.format(what, a_noise))
    xi_h1_db, xi_min_db = _number(xi_h1_db, what, 'xi_h1_db'), _number(xi_min_db, what, 'xi_min_db')
    floor_db, gamma_max = _number(floor_db, what, 'floor_db'), _number(gamma_max, what, 'gamma_max')
    if abs(xi_h1_db) > 300.0 or abs(xi_min_db) > 300.0:
        raise ValueError(' - ERROR, {}: xi_h1_db and xi_min_db must be within +-300 dB'.format(what))
    if not 0.0 <= floor_db <= 300.0:
        raise ValueError(' - ERROR, {}: floor_db (the largest attenuation, in dB) must be in [0, 300], got {!r}'.format(what, floor_db))
    if not gamma_max > 0.0:
        raise ValueError(' - ERROR, {}: gamma_max must be positive, got {!r}'.format(what, gamma_max))
    return _vc.DenoiseCfg(RULES[rule], int(n_init), a_spp, a_noise, a_dd, 10.0 ** (xi_h1_db / 10.0), 10.0 ** (xi_min_db / 10.0),
                          10.0 ** (-floor_db / 20.0), gamma_max)


def _check_noise0(what, noise0, B, n_bins):
    if noise0 is not None and (getattr(noise0, 'ndim', 0) != 2 or tuple(noise0.shape) != (B, n_bins)):
        raise ValueError(' - ERROR, {}: noise0 must be [{}, {}]'.format(what, B, n_bins))


def _as_cuda_f32(t):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device='cuda', dtype=torch.float32).contiguous()


def _noise_gain_launch(power, d_nf, noise0, cfg, return_noise):
    """vc_noise_gain_f32 on validated device tensors: (gain, noise or None); no host check, copy or wait in here."""
    import ctypes
    import torch
    B, Fmax, n_bins = power.shape
    gain = torch.empty_like(power)
    noise = torch.empty_like(power) if return_noise else None
    _vc.check(_vc.lib().vc_noise_gain_f32(_vc.ptr(power), _vc.ptr(d_nf), _vc.ptr(noise0), B, Fmax, n_bins, ctypes.byref(cfg),
                                          _vc.ptr(gain), _vc.ptr(noise), _vc.current_stream()))
    return gain, noise


def noise_gain_batch(power, n_frames, rule='logmmse', noise0=None, n_init=8, a_spp=None, a_noise=None, a_dd=0.98, xi_h1_db=15,
                     xi_min_db=-25, floor_db=20, gamma_max=1000.0, return_noise=False):
    """The suppression gain of a ragged batch of power spectrograms (vc_noise_gain_f32).

    power [B, F, bins] float32, linear (audio_lib.stft_power_batch); n_frames: host integers or an int32 [B] device tensor
    (None = all F).  rule: 'logmmse' or 'wiener'.  noise0 [B, bins]: the noise power to start from (None: the mean of the
    first n_init frames, so the recording should open with noise alone).  a_spp, a_noise: the tracker's smoothing constants
    (None: ``smoothing(80, 16000)``, the shipped hop); a_dd: the decision-directed weight; xi_h1_db: the tracker's fixed prior
    SNR; xi_min_db: the lower limit of the a-priori SNR; floor_db: the largest attenuation; gamma_max: the limit of the
    a-posteriori SNR.  Returns gain [B, F, bins] on the device, or (gain, noise) with return_noise; rows at or beyond an
    utterance's frame count are 0.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'noise_gain_batch'
    if getattr(power, 'ndim', 0) != 3 or min(power.shape) < 1 or not 2 <= power.shape[2] <= 2049:
        raise ValueError(' - ERROR, {}: power must be [B, F, bins] with 2 <= bins <= 2049'.format(what))
    B, Fmax, n_bins = (int(v) for v in power.shape)
    if B > 65535:
        raise ValueError(' - ERROR, {}: at most 65535 utterances'.format(what))
    if n_frames is not None and torch.is_tensor(n_frames) and n_frames.is_cuda:
        if n_frames.dtype != torch.int32 or tuple(n_frames.shape) != (B,):
            raise ValueError(' - ERROR, {}: n_frames on the device must be int32 [{}]'.format(what, B))
    elif n_frames is not None:
        h = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > Fmax:
            raise ValueError(' - ERROR, {}: n_frames must be {} integers in [0, {}]'.format(what, B, Fmax))
    _check_noise0(what, noise0, B, n_bins)
    cfg = gain_cfg(what, rule, n_init, a_spp, a_noise, a_dd, xi_h1_db, xi_min_db, floor_db, gamma_max)
    if not torch.cuda.is_available():
        raise _vc.VCError('noise_gain_batch needs a GPU (no CPU fallback)')
    import audio_lib
    d_nf = None if n_frames is None else audio_lib._int32_device(n_frames, B, 'n_frames')
    gain, noise = _noise_gain_launch(_as_cuda_f32(power), d_nf, None if noise0 is None else _as_cuda_f32(noise0), cfg,
                                     bool(return_noise))
    return (gain, noise) if return_noise else gain


def check_gain_keywords(what, kw, hop_length, sr):
    """The noise_gain_batch keywords of a denoise request (a dict) checked on the host: (cfg, noise0, return_noise)."""
    bad = sorted(set(kw) - set(GAIN_KEYS))
    if bad:
        raise ValueError(' - ERROR, {}: unknown noise-suppression keyword(s) {}; known: {}'.format(what, ', '.join(bad),
                                                                                                ', '.join(GAIN_KEYS)))
    args = {k: v for k, v in kw.items() if k not in ('noise0', 'return_noise')}
    return gain_cfg(what, hop_length=hop_length, sr=sr, **args), kw.get('noise0'), bool(kw.get('return_noise', False))


def _denoise_launch(plan, wav, d_len, d_nf, Fmax, cfg, noise0, return_noise):
    """power, gain, filter on validated device tensors: the namedtuple of denoise_batch."""
    import audio_lib
    power, d_fout = audio_lib._stft_power_launch(plan, wav, d_len, d_nf, Fmax)
    gain, noise = _noise_gain_launch(power, d_fout, noise0, cfg, return_noise)
    y = audio_lib._stft_filter_launch(plan, wav, d_len, gain, d_fout)
    return _DENOISE_NT(y, gain, noise, d_fout)


def denoise_batch(wav, lens, sr=16000, win_length=400, hop_length=80, n_fft=None, n_frames=None, **gain_kw):
    """Stationary noise suppressed in a ragged batch of waveforms: y = istft(G * stft(wav)) with G from noise_gain_batch on
    |stft(wav)|^2.  Three launches and the overlap-add.

    wav [B, Lmax] float32 (numpy or tensor); lens: the sample counts, host integers or an int32 [B] device tensor (None =
    all Lmax); n_frames as in audio_lib.stft_power_batch; the other keywords are noise_gain_batch's, with a_spp / a_noise
    defaulting to ``smoothing(hop_length, sr)``.
    Returns a namedtuple of device tensors: y [B, hop_length * (F - 1)] with F = 1 + Lmax // hop_length (hop_length *
    (frames - 1) samples per utterance, zeros beyond; a row of zeros for an utterance shorter than the reflect padding),
    gain [B, F, bins], noise (the tracked noise power, None unless return_noise) and n_frames int32 [B], the frame counts
    the device used.  Nothing is copied back and the host waits for nothing."""
    import torch
    import audio_lib
    what = 'denoise_batch'
    B, Lmax, Fmax, plan_key = audio_lib._check_stft_wave_args(what, wav, lens, n_frames, win_length, hop_length, n_fft)
    if Fmax < 2:
        raise ValueError(' - ERROR, {}: wav must hold at least hop_length = {} samples'.format(what, plan_key[1]))
    cfg, noise0, return_noise = check_gain_keywords(what, gain_kw, plan_key[1], sr)
    _check_noise0(what, noise0, B, 1 + plan_key[2] // 2)
    if not torch.cuda.is_available():
        raise _vc.VCError('denoise_batch needs a GPU (no CPU fallback)')
    plan = audio_lib._get_voc_plan(*plan_key)
    wav, d_len, d_nf = audio_lib._stft_wave_upload(wav, lens, n_frames, B, Lmax)
    return _denoise_launch(plan, wav, d_len, d_nf, Fmax, cfg, None if noise0 is None else _as_cuda_f32(noise0), return_noise)
