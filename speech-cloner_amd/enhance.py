"""Noise suppression and dereverberation on the device: what is taken out of a waveform before it is analysed or converted.

Noise suppression (include/vc_hip.h, "Noise suppression"): stationary noise.  Three launches and the overlap-add:

    power   P = |stft(x)|^2                                     audio_lib.stft_power_batch   (vc_stft_power_f32)
    gain    noise tracker + suppression rule, one scan in time  noise_gain_batch             (vc_noise_gain_f32)
    filter  y = istft(G * stft(x))                              audio_lib.stft_filter_batch  (vc_stft_filter_f32)

The tracker is Gerkmann & Hendriks' speech-presence-probability estimator (2012), the rule Ephraim & Malah's log-MMSE
amplitude estimator (or the Wiener gain) on the decision-directed a-priori SNR with Cappe's lower limit.  The defaults are
the literature's, carried to this project's 5 ms hop (``smoothing``); nobody has listened to anything they produce.
tests/denoise_ref.py restates both new launches in numpy.

Dereverberation (include/vc_hip.h, "Dereverberation"): late reverberation, which follows the speech and which no noise
tracker sees.  Weighted prediction error (Nakatani et al. 2010; nara_wpe's formulation): per bin a delayed linear predictor
over past frames, re-weighted least squares, subtracted.  It sits in front of the noise suppression:

    stft    Z = stft(x), planar and bin-major                   audio_lib.stft_complex_batch   (vc_stft_complex_f32)
    wpe     the solver, one workgroup per (utterance, bin)      wpe_batch                      (vc_wpe_f32)
    istft   y = istft(Z'), then the overlap-add                 audio_lib.istft_complex_batch  (vc_istft_complex_f32)

Delay and taps are carried to this project's 5 ms hop (``wpe_defaults``); nobody has listened to anything this produces.
tests/dereverb_ref.py restates the three launches in numpy.

There is no CPU fallback: without a GPU every call raises."""
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


# --------------------------------------------------------------------------- dereverberation
WPE_MAX_TAPS, WPE_MAX_DELAY, WPE_MAX_ITERATIONS, WPE_MAX_CONTEXT = 32, 64, 16, 8     # include/vc_hip.h, vc_wpe_f32
WPE_KEYS = ('taps', 'delay', 'iterations', 'context', 'floor_db', 'load', 'return_taps')
_WPE_NT = collections.namedtuple('wpe', 're im status taps')
_DEREVERB_NT = collections.namedtuple('dereverb', 'y n_frames status taps')


def wpe_defaults(hop_length, sr, win_length, span_ms=80.0):
    """(taps, delay) of the WPE predictor for this framing: delay = ceil(win_length / hop_length), taps = round(span_ms * sr /
    1000 / hop_length), both clamped to the launch's limits (32 taps, 64 frames).

    A prediction that starts inside the analysis window of the frame it predicts cancels the speech itself: frames closer
    than one window share samples with it, so the delay is counted in windows, not in frames.  nara_wpe's 10 taps and delay
    3 are meant for an 8 ms hop: 80 ms of history behind a window.  This is ``smoothing``'s argument made for WPE -- a constant
    that was chosen at another hop is a time, and is carried over as a time.  At the shipped 400 / 80 / 16 kHz it gives
    (16, 5)."""
    for v, name in ((hop_length, 'hop_length'), (sr, 'sr'), (win_length, 'win_length'), (span_ms, 'span_ms')):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v <= 0:
            raise ValueError(' - ERROR, wpe_defaults: {} must be a positive number, got {!r}'.format(name, v))
    delay = int(math.ceil(float(win_length) / float(hop_length)))
    taps = int(round(float(span_ms) * float(sr) / 1000.0 / float(hop_length)))
    return min(max(taps, 1), WPE_MAX_TAPS), min(max(delay, 1), WPE_MAX_DELAY)


def _wpe_int(v, what, name, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(' - ERROR, {}: {} must be an integer in [{}, {}], got {!r}'.format(what, name, lo, hi, v))
    return int(v)


def wpe_cfg(what, taps=None, delay=None, iterations=3, context=1, floor_db=-60.0, load=1e-8, hop_length=80, sr=16000,
            win_length=400):
    """The checked vc_wpe_cfg of a wpe_batch call (ValueError otherwise; no GPU).  taps / delay None: those of
    ``wpe_defaults(hop_length, sr, win_length)``.  floor_db: the floor of the weight relative to the bin's mean power, in dB
    (in [-200, 0]); load: the diagonal loading relative to the mean of the diagonal (in [0, 1])."""
    d_taps, d_delay = wpe_defaults(hop_length, sr, win_length)
    taps = d_taps if taps is None else _wpe_int(taps, what, 'taps', 1, WPE_MAX_TAPS)
    delay = d_delay if delay is None else _wpe_int(delay, what, 'delay', 1, WPE_MAX_DELAY)
    iterations = _wpe_int(iterations, what, 'iterations', 1, WPE_MAX_ITERATIONS)
    context = _wpe_int(context, what, 'context', 0, WPE_MAX_CONTEXT)
    floor_db, load = _number(floor_db, what, 'floor_db'), _number(load, what, 'load')
    if not -200.0 <= floor_db <= 0.0:
        raise ValueError(' - ERROR, {}: floor_db (relative to the mean power, in dB) must be in [-200, 0], got {!r}'.format(what, floor_db))
    if not 0.0 <= load <= 1.0:
        raise ValueError(' - ERROR, {}: load must be in [0, 1], got {!r}'.format(what, load))
    return _vc.WpeCfg(taps, delay, iterations, context, 10.0 ** (floor_db / 10.0), load)


def wpe_max_frames(taps):
    """The most frames vc_wpe_f32 takes with this many taps (a bin's frames live in LDS): vc_wpe_max_frames, host only."""
    return int(_vc.lib().vc_wpe_max_frames(_wpe_int(taps, 'wpe_max_frames', 'taps', 1, WPE_MAX_TAPS)))


def check_wpe_keywords(what, kw, hop_length, sr, win_length):
    """The wpe_batch keywords of a dereverberation request (a dict) checked on the host: (cfg, return_taps)."""
    bad = sorted(set(kw) - set(WPE_KEYS))
    if bad:
        raise ValueError(' - ERROR, {}: unknown dereverberation keyword(s) {}; known: {}'.format(what, ', '.join(bad),
                                                                                              ', '.join(WPE_KEYS)))
    args = {k: v for k, v in kw.items() if k != 'return_taps'}
    return wpe_cfg(what, hop_length=hop_length, sr=sr, win_length=win_length, **args), bool(kw.get('return_taps', False))


def _check_wpe_frames(what, Fmax, cfg):
    cap = wpe_max_frames(cfg.taps)
    if Fmax > cap:
        raise ValueError(' - ERROR, {}: {} frames exceed the {} that {} taps leave room for (vc_wpe_max_frames)'.format(
            what, Fmax, cap, cfg.taps))


def _wpe_launch(re, im, d_nf, cfg, return_taps):
    """vc_wpe_f32 on validated device tensors: the namedtuple of wpe_batch; no host check, copy or wait in here."""
    import ctypes
    import torch
    B, n_bins, Fmax = re.shape
    out_re, out_im = torch.empty_like(re), torch.empty_like(im)
    status = torch.empty((B, n_bins), dtype=torch.int32, device=re.device)
    taps = torch.empty((B, n_bins, cfg.taps, 2), dtype=torch.float32, device=re.device) if return_taps else None
    _vc.check(_vc.lib().vc_wpe_f32(_vc.ptr(re), _vc.ptr(im), _vc.ptr(d_nf), B, n_bins, Fmax, ctypes.byref(cfg), _vc.ptr(out_re),
                                   _vc.ptr(out_im), _vc.ptr(taps), _vc.ptr(status), _vc.current_stream()))
    return _WPE_NT(out_re, out_im, status, taps)


def wpe_batch(re, im, n_frames, taps=None, delay=None, iterations=3, context=1, floor_db=-60.0, load=1e-8, return_taps=False):
    """WPE dereverberation of a ragged batch of spectra (vc_wpe_f32): spectra in, spectra out.

    re, im [B, bins, F] float32, planar and bin-major (audio_lib.stft_complex_batch); n_frames: host integers or an int32 [B]
    device tensor (None = all F).  taps, delay: the predictor's length and the frames between its newest frame and the
    predicted one (None: ``wpe_defaults(80, 16000, 400)``, the shipped framing); iterations: re-weighting passes; context:
    the weight is the power averaged over +-context frames; floor_db: the weight's floor relative to the bin's mean power;
    load: diagonal loading relative to the mean of the diagonal.
    Returns a namedtuple of device tensors: re, im [B, bins, F] (frames at or beyond an utterance's count are 0), status int32
    [B, bins] (0 solved; 1 the factorisation met a pivot that was not positive -- an all-zero bin is one; 2 no more frames
    than the delay; with 1 or 2 the bin is passed through unchanged) and taps [B, bins, taps, 2] (None unless return_taps).
    F is limited to wpe_max_frames(taps), at least 6121 (30 s at a 5 ms hop).  Nothing is copied back and the host waits
    for nothing."""
    import torch
    import audio_lib
    what = 'wpe_batch'
    B, _, Fmax = audio_lib._check_spectrum_args(what, re, im, n_frames)
    cfg = wpe_cfg(what, taps, delay, iterations, context, floor_db, load)
    _check_wpe_frames(what, Fmax, cfg)
    if not torch.cuda.is_available():
        raise _vc.VCError('wpe_batch needs a GPU (no CPU fallback)')
    d_nf = None if n_frames is None else audio_lib._int32_device(n_frames, B, 'n_frames')
    return _wpe_launch(audio_lib._spectrum_upload(re), audio_lib._spectrum_upload(im), d_nf, cfg, bool(return_taps))


def _dereverb_launch(plan, wav, d_len, d_nf, Fmax, cfg, return_taps):
    """stft, wpe, istft on validated device tensors: the namedtuple of dereverb_batch."""
    import audio_lib
    re, im, d_fout = audio_lib._stft_complex_launch(plan, wav, d_len, d_nf, Fmax)
    r = _wpe_launch(re, im, d_fout, cfg, return_taps)
    y = audio_lib._istft_complex_launch(plan, r.re, r.im, d_fout)
    return _DEREVERB_NT(y, d_fout, r.status, r.taps)


def dereverb_batch(wav, lens, sr=16000, win_length=400, hop_length=80, n_fft=None, n_frames=None, **wpe_kw):
    """Late reverberation taken out of a ragged batch of waveforms: y = istft(wpe(stft(wav))).  Three launches and the
    overlap-add.

    wav, lens, n_frames: as denoise_batch's; the other keywords are wpe_batch's, with taps / delay defaulting to
    ``wpe_defaults(hop_length, sr, win_length)``.
    Returns a namedtuple of device tensors: y [B, hop_length * (F - 1)] with F = 1 + Lmax // hop_length (hop_length *
    (frames - 1) samples per utterance, zeros beyond; a row of zeros for an utterance shorter than the reflect padding),
    n_frames int32 [B], the frame counts the device used, status int32 [B, bins] and taps (None unless return_taps), as
    wpe_batch's.  Nothing is copied back and the host waits for nothing."""
    import torch
    import audio_lib
    what = 'dereverb_batch'
    B, Lmax, Fmax, plan_key = audio_lib._check_stft_wave_args(what, wav, lens, n_frames, win_length, hop_length, n_fft)
    if Fmax < 2:
        raise ValueError(' - ERROR, {}: wav must hold at least hop_length = {} samples'.format(what, plan_key[1]))
    cfg, return_taps = check_wpe_keywords(what, wpe_kw, plan_key[1], sr, plan_key[0])
    _check_wpe_frames(what, Fmax, cfg)
    if not torch.cuda.is_available():
        raise _vc.VCError('dereverb_batch needs a GPU (no CPU fallback)')
    plan = audio_lib._get_voc_plan(*plan_key)
    wav, d_len, d_nf = audio_lib._stft_wave_upload(wav, lens, n_frames, B, Lmax)
    return _dereverb_launch(plan, wav, d_len, d_nf, Fmax, cfg, return_taps)
