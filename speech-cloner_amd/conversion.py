"""Conversion driver helpers with the surface of the reference's ``test.py``.

Mirrors /root/reference/test.py:46-306: ``compound`` (stitching of half-overlapped window
predictions), ``conversion`` (non-overlapping windows) and ``conversion2`` (two passes shifted by
half a window, stitched) -- the pure integer framing that turns an utterance's features into
[N, n_timesteps, C] batches for ``decoder.predict`` and back, followed by the Griffin-Lim vocoder
(audio_lib.from_power_to_wav on the GPU, test.py:146-168).  Plotting, audio playback and wav
writing (test.py:28-43, 171-188) are UI side effects and out of scope.  ``vocoder``: 'default' =
audio_lib.from_power_to_wav, any callable with that signature, or None to skip audio synthesis
(``y_wav_true`` / ``y_wav_pred`` are then None).  ``momentum`` (default 0.0): fast Griffin-Lim; a
callable receives ``momentum=`` only when it is not 0, so a reference-signature vocoder keeps working.

``convert_batch`` is the same conversion for a ragged batch of waveforms with nothing leaving the
device: front-end -> vc_cut_windows -> encoder + decoder over window chunks -> vc_compound_stitch ->
vc_phase_init -> Griffin-Lim, all tables computed on the host from the lengths before the first
launch (``convert_plan``) and uploaded once; it returns cuda tensors.  ``wav_sr`` / ``out_sr`` put
audio_lib's device resampler in front of and behind that chain for audio at another sample rate.

``convert_duration_batch`` is ``convert_batch`` with the timing changed as well: between the stitch
and the vocoder, ``duration_map_batch`` (vc_duration_map: an integer time map from a segment table and per-class rates or
explicit lengths) and ``time_warp_batch`` (vc_time_warp) resample the stitched spectra; the output lengths stay on the
device.  ``duration_stats_batch`` / ``duration_ratios`` turn two speakers' segment tables into the rate table.

``convert_pitch_batch`` is ``convert_batch`` with the melody set as well: behind the vocoder the
converted waveform's F0 is tracked and ``pitch_shift_batch``'s launches (vc_psola_plan, vc_psola_ola_f32: overlap-add of
grains placed by integrating the track) move it by a ratio, to a given contour or to the source's own.  ``pitch_tables``
builds the launch's two Q16 tables from a track; ``f0_stats_batch`` / ``f0_transform`` map a contour between speakers.

``convert_diff_batch`` makes the waveform without a vocoder: ``diff_gain_batch``
(vc_spectral_diff_gain_f32) turns the converted and the source spectrum into a smoothed, clamped gain per frame and bin, and
``audio_lib.stft_filter_batch`` (vc_stft_filter_f32) filters the source recording by it in one STFT / ISTFT pass, optionally
after ``pitch_shift_batch``'s launches moved the source's fundamental.

``convert_diff_duration_batch`` is ``convert_diff_batch`` with the timing changed as well: the FILTERED
waveform is moved along ``duration_map_batch``'s time map by ``time_scale_batch`` (vc_wsola_plan, vc_wsola_ola_f32:
waveform-similarity overlap-add -- copied grains, each chosen near the map so that it continues its predecessor), which
keeps the recording's local phase; ``wsola_plan_batch`` returns the grain positions alone.
"""
from collections import namedtuple

import numpy as np


def compound_index(N, T):
    """Source of every output frame of ``compound``: int arrays (which, window, frame) where
    which = 0 selects y0 and 1 selects y1.  Closed form of the loop at test.py:58-80:
    y0[0][:T-q], then alternately y1[i][q:T-q], y0[i+1][q:T-q], finally y0[N-1][q:], q = T//4."""
    q = T // 4
    fr = np.arange(T)
    head, mid, tail = fr[:-q], fr[q:-q], fr[q:]
    which, win, frame = [np.zeros(len(head), np.int64)], [np.zeros(len(head), np.int64)], [head]
    i_0, i_1 = 1, 0
    while i_1 < N - 1 or i_0 < N - 1:
        if i_1 < N - 1:
            which.append(np.ones(len(mid), np.int64)); win.append(np.full(len(mid), i_1, np.int64)); frame.append(mid)
            i_1 += 1
        if i_0 < N - 1:
            which.append(np.zeros(len(mid), np.int64)); win.append(np.full(len(mid), i_0, np.int64)); frame.append(mid)
            i_0 += 1
    which.append(np.zeros(len(tail), np.int64)); win.append(np.full(len(tail), N - 1, np.int64)); frame.append(tail)
    return np.concatenate(which), np.concatenate(win), np.concatenate(frame)


def compound(y0, y1):
    """test.py:46-84.  y0 [N, T, X], y1 [N-1, T, X] -> [N*T, X]: the centre half of every window
    (three quarters at both ends), alternating between the two passes."""
    N, T = y0.shape[0], y0.shape[1]
    which, win, frame = compound_index(N, T)
    if y1.shape[0] < N - 1:
        raise IndexError(' - ERROR, compound: y1 must hold N-1 windows')
    both = np.concatenate([y0, y1[:max(N - 1, 0)]], axis=0)
    return both[win + which * N, frame]


def window_plan(n_frames, cfg_d, t_s, t_e):
    """Integer window arithmetic of test.py:92-119 / 211-238.  Returns (pad_len, n_s, n_e) for an
    utterance of ``n_frames`` frames; raises like the reference when the span is empty."""
    hop = cfg_d['hop_length']
    n_times = cfg_d['n_timesteps']
    pad_len = 0
    if n_frames % n_times != 0:
        pad_len = n_times - (n_frames % n_times)
    n_hop_s = t_s * cfg_d['sample_rate'] // hop
    n_hop_e = t_e * cfg_d['sample_rate'] // hop
    n_hop_e = min(n_hop_e, n_frames + pad_len)
    n_delta = n_times * ((n_hop_e - n_hop_s) // n_times)
    n_s = n_hop_s
    n_e = n_hop_s + n_delta
    if n_e <= n_s:
        raise Exception(' - ERROR, translate: n_e <= n_s.')
    return pad_len, n_s, n_e


def _pad_all(mfcc, mel, stft, pad_len):
    if pad_len == 0:
        return mfcc, mel, stft
    print('Padding!!')
    out = []
    for a in (mfcc, mel, stft):
        out.append(np.concatenate([a, np.zeros((pad_len, a.shape[1]))], axis=0))
    print(out[0].shape, out[1].shape, out[2].shape)
    return out


def _check_momentum(momentum):
    import audio_lib
    return audio_lib.check_momentum(momentum)


def _vocode(vocoder, stft_true, stft_pred, cfg_d, n_iter, realse, giffin_lim_input, momentum=0.0):
    if vocoder is None:
        return None, None
    if vocoder == 'default':
        import audio_lib
        vocoder = audio_lib.from_power_to_wav
    kw = dict(P_dB_norm_factor=cfg_d['P_dB_norm_factor'], pre_emphasis=cfg_d['pre_emphasis'],
              hop_length=cfg_d['hop_length'], win_length=cfg_d['win_length'],
              mean_abs_amp_norm=15 * cfg_d['mean_abs_amp_norm'], n_iter=n_iter, n_fft=cfg_d['n_fft'])
    if momentum != 0.0:
        kw['momentum'] = momentum
    y_true = vocoder(stft_true, realse=1.0, **kw) if giffin_lim_input else None
    return y_true, vocoder(stft_pred, realse=realse, **kw)


def conversion2(decoder, mfcc, mel, stft, cfg_d, t_s=5, t_e=60, n_iter=200, output_path='./output',
                file_name='y_wav', realse=1.0, save_output=False, giffin_lim_input=True, play_conversion=False,
                vocoder='default', momentum=0.0):
    """test.py:87-201: half-overlapped double pass + ``compound``."""
    momentum = _check_momentum(momentum)
    n_times = cfg_d['n_timesteps']
    pad_len, n_s, n_e = window_plan(mfcc.shape[0], cfg_d, t_s, t_e)
    mfcc, mel, stft = _pad_all(mfcc, mel, stft, pad_len)

    mfcc_input0 = mfcc[n_s:n_e].reshape((-1, n_times, mfcc.shape[-1]))
    y_pred0 = decoder.predict(mfcc_input0)
    if n_e - n_s > n_times:
        half = n_times // 2
        mfcc_input1 = mfcc[(n_s + half):(n_e - half)].reshape((-1, n_times, mfcc.shape[-1]))
        y_pred1 = decoder.predict(mfcc_input1)
        mel_pred = compound(y_pred0.y_mel, y_pred1.y_mel)
        stft_pred = compound(y_pred0.y_stft, y_pred1.y_stft)
        phn_pred = compound(y_pred0.y_phn, y_pred1.y_phn)
    else:
        mel_pred = y_pred0.y_mel.reshape((-1, y_pred0.y_mel.shape[-1]))
        stft_pred = y_pred0.y_stft.reshape((-1, y_pred0.y_stft.shape[-1]))
        phn_pred = y_pred0.y_phn.reshape((-1, y_pred0.y_phn.shape[-1]))

    mel_true = mel[n_s:n_e]
    stft_true = stft[n_s:n_e]
    y_wav_true, y_wav_pred = _vocode(vocoder, stft_true, stft_pred, cfg_d, n_iter, realse, giffin_lim_input,
                                     momentum)
    ret_tuple = namedtuple('conversion', 'y_wav_true y_wav_pred mel_true mel_pred stft_true stft_pred phn_pred')
    return ret_tuple(y_wav_true, y_wav_pred, mel_true, mel_pred, stft_true, stft_pred, phn_pred)


def conversion(decoder, mfcc, mel, stft, cfg_d, t_s=5, t_e=60, n_iter=200, output_path='./output',
               file_name='y_wav', realse=1.0, save_output=False, giffin_lim_input=True, play_conversion=False,
               vocoder='default', momentum=0.0):
    """test.py:206-306: single pass over non-overlapping windows."""
    momentum = _check_momentum(momentum)
    n_times = cfg_d['n_timesteps']
    pad_len, n_s, n_e = window_plan(mfcc.shape[0], cfg_d, t_s, t_e)
    mfcc, mel, stft = _pad_all(mfcc, mel, stft, pad_len)
    y_pred = decoder.predict(mfcc[n_s:n_e].reshape((-1, n_times, mfcc.shape[-1])))
    mel_true = mel[n_s:n_e]
    mel_pred = y_pred.y_mel.reshape((-1, y_pred.y_mel.shape[-1]))
    stft_true = stft[n_s:n_e]
    stft_pred = y_pred.y_stft.reshape((-1, y_pred.y_stft.shape[-1]))
    y_wav_true, y_wav_pred = _vocode(vocoder, stft_true, stft_pred, cfg_d, n_iter, realse, giffin_lim_input,
                                     momentum)
    ret_tuple = namedtuple('conversion', 'y_wav_true y_wav_pred mel_true mel_pred stft_true stft_pred')
    return ret_tuple(y_wav_true, y_wav_pred, mel_true, mel_pred, stft_true, stft_pred)


# --------------------------------------------------------------------------- batched, device-resident
_PLAN_NT = namedtuple('convert_plan', 'B T Fout W n_src n_s n_e N n_clip n_out win_tab utt_tab true_tab')
_BATCH_NT = namedtuple('convert_batch', 'y_wav_true y_wav_pred n_samples mel_true mel_pred stft_true stft_pred '
                                        'phn_pred n_frames')


def convert_plan(lens, cfg_d, t_s=0, t_e=60, two_pass=True):
    """Host tables of ``convert_batch`` for utterances of ``lens`` samples (pure integer work, no GPU):
      n_src [B]       front-end frames 1 + len // hop
      n_s, n_e, N [B] ``window_plan`` per utterance and its window count (n_e - n_s) // T
      n_clip [B]      min(n_src, n_e): source rows at or beyond it read as zeros (the reference's padding, and its cut at t_e)
      n_out [B]       N * T output frames; Fout = max(n_out)
      win_tab [W, 2]  (utterance, first frame) of every window: per utterance its N pass-0 windows from n_s, then, with
                      two_pass and N > 1, its N - 1 pass-1 windows from n_s + T // 2
      utt_tab [B, 3]  (first pass-0 window, first pass-1 window or -1, N)
      true_tab [B, 2] (utterance, n_s): the one Fout-row "window" that cuts mel_true / stft_true
    An empty span raises the reference's error (test.py:117-119) with the utterance's index."""
    T, hop = int(cfg_d['n_timesteps']), int(cfg_d['hop_length'])
    if T <= 0 or T % 4 != 0:
        raise ValueError(' - ERROR, convert_batch: n_timesteps must be a positive multiple of 4 (compound cuts quarters)')
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    B = len(lens)
    n_src = 1 + lens // hop
    n_s, n_e, N = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    win, utt = [], []
    for b in range(B):
        try:
            _, n_s[b], n_e[b] = window_plan(int(n_src[b]), cfg_d, t_s, t_e)
        except Exception as e:
            raise Exception('{} (utterance {} of the batch, {} frames)'.format(e, b, int(n_src[b]))) from None
        N[b] = (n_e[b] - n_s[b]) // T
        w0 = len(win)
        win += [(b, n_s[b] + i * T) for i in range(N[b])]
        w1 = -1
        if two_pass and N[b] > 1:
            w1 = len(win)
            win += [(b, n_s[b] + T // 2 + i * T) for i in range(N[b] - 1)]
        utt.append((w0, w1, N[b]))
    n_out = N * T
    i32 = lambda a, shape: np.asarray(a, dtype=np.int32).reshape(shape)
    return _PLAN_NT(B, T, int(n_out.max()), len(win), i32(n_src, (B,)), i32(n_s, (B,)), i32(n_e, (B,)), i32(N, (B,)),
                    i32(np.minimum(n_src, n_e), (B,)), i32(n_out, (B,)), i32(win, (-1, 2)), i32(utt, (B, 3)),
                    i32(np.stack([np.arange(B), n_s], 1), (B, 2)))


def cut_windows(src, win_tab, n_frames, T, out=None):
    """vc_cut_windows (include/vc_hip.h): src [B, Fmax, C] float32 cuda -> [W, T, C]; win_tab int32 [W, 2] cuda
    (utterance, first frame); rows at or beyond n_frames[utterance] (int32 [B] cuda, or None) are zeros."""
    import torch
    import _vc
    B, Fmax, C = src.shape
    W = win_tab.shape[0]
    if out is None:
        out = torch.empty((W, int(T), C), dtype=torch.float32, device=src.device)
    _vc.check(_vc.lib().vc_cut_windows(_vc.ptr(src), _vc.ptr(win_tab), _vc.ptr(n_frames), B, Fmax, W, int(T), C,
                                       _vc.ptr(out), _vc.current_stream()))
    return out


def compound_stitch(src, utt_tab, Fout, P_dB_norm_factor=None, out=None, amp=None):
    """vc_compound_stitch (include/vc_hip.h): window batch src [W, T, C] (float32 or bfloat16 cuda) -> [B, Fout, C]
    float32; utt_tab int32 [B, 3] cuda.  With P_dB_norm_factor also the vocoder's magnitude (realse == 1): returns
    (stitched, amp)."""
    import torch
    import _vc
    W, T, C = src.shape
    B = utt_tab.shape[0]
    if src.dtype not in (torch.float32, torch.bfloat16):
        src = src.float()
    if out is None:
        out = torch.empty((B, int(Fout), C), dtype=torch.float32, device=src.device)
    if P_dB_norm_factor is not None and amp is None:
        amp = torch.empty((B, int(Fout), C), dtype=torch.float32, device=src.device)
    _vc.check(_vc.lib().vc_compound_stitch(_vc.ptr(src), _vc.VC_BF16 if src.dtype == torch.bfloat16 else _vc.VC_F32,
                                           _vc.ptr(utt_tab), B, W, T, C, int(Fout), _vc.ptr(out), _vc.ptr(amp),
                                           float(P_dB_norm_factor or 0.0), _vc.current_stream()))
    return out if P_dB_norm_factor is None else (out, amp)


def _numpy_phase(plan, n_bins, both):
    """The reference's draws (audio_lib.py:255) from the global generator, per utterance in batch order, the true
    spectrum's first, then the predicted one's: what a loop of conversion2 calls draws."""
    ph = np.zeros((2 if both else 1, plan.B, plan.Fout, n_bins), dtype=np.float32)
    for b in range(plan.B):
        n = int(plan.n_out[b])
        for k in range(ph.shape[0]):
            ph[k, b, :n] = (np.pi * np.random.rand(n_bins, n)).T
    return ph


_HOST_NT = namedtuple('convert_host', 'plan B hop n_fft n_bins h_lens h_lens_in h_nsamp utt_ids res_in res_out window_batch denoise '
                                      'dereverb', defaults=(None,))
_UP_NT = namedtuple('convert_upload', 'wav d_lens d_clip d_nout d_ids d_win d_utt d_true d_extra')


def _need_cfg(cfg_d, what):
    if cfg_d is None:
        raise ValueError(' - ERROR, {}: cfg_d (the data-set configuration) is required'.format(what))


def _need_gpu(what):
    """The last check of every entry point: nothing before it touches the device."""
    import torch
    import _vc
    if not torch.cuda.is_available():
        raise _vc.VCError('{} needs a GPU (no CPU fallback)'.format(what))


def _check_phase(phase, what, shape=None, allowed=('device', 'spsi'), frames='Fout', note=''):
    """phase= of a conversion: one of the strings ``allowed``, or an array of ``shape`` (None before the plan is known: only
    the string is checked then)."""
    if isinstance(phase, str):
        if phase not in allowed:
            raise ValueError(' - ERROR, {}: phase must be {} or a [B, {}, bins] array{}, got {!r}'.format(
                what, ', '.join(repr(a) for a in allowed), frames, note, phase))
    elif shape is not None and tuple(phase.shape) != tuple(shape):
        raise ValueError(' - ERROR, {}: phase must be [{}, {}, {}]'.format(what, *shape))


def _phase_upload(phase):
    """A phase given as an array, on the device; a string passes through (the vocoder tail makes that phase)."""
    import torch
    if isinstance(phase, str):
        return phase
    if not torch.is_tensor(phase):
        phase = torch.from_numpy(np.ascontiguousarray(phase, dtype=np.float32))
    return phase.to(device='cuda', dtype=torch.float32).contiguous()


def _check_denoise(what, denoise, cfg_d, B):
    """denoise= of a conversion, on the host: None for None / False, else (vc_denoise_cfg, noise0 or None).  True means
    enhance.denoise_batch's defaults; a dict holds its noise-suppression keywords (enhance.GAIN_KEYS without return_noise:
    the conversion returns no noise track)."""
    if denoise is None or denoise is False:
        return None
    import enhance
    if denoise is True:
        denoise = {}
    if not isinstance(denoise, dict):
        raise ValueError(' - ERROR, {}: denoise must be None, True or a dict of enhance.denoise_batch keywords, got {!r}'.format(
            what, denoise))
    if 'return_noise' in denoise:
        raise ValueError(' - ERROR, {}: denoise: return_noise is not offered here (call enhance.denoise_batch)'.format(what))
    n_fft = cfg_d['n_fft'] or cfg_d['win_length']
    cfg, noise0, _ = enhance.check_gain_keywords(what + ': denoise', denoise, int(cfg_d['hop_length']), cfg_d['sample_rate'])
    enhance._check_noise0(what + ': denoise', noise0, B, 1 + n_fft // 2)
    return cfg, noise0


def _check_dereverb(what, dereverb, cfg_d, Lmax):
    """dereverb= of a conversion, on the host: None for None / False, else the vc_wpe_cfg.  True means
    enhance.dereverb_batch's defaults for the data set's framing; a dict holds enhance.wpe_batch's keywords (enhance.WPE_KEYS
    without return_taps: the conversion returns no predictor).  Lmax: the longest waveform at the model's rate."""
    if dereverb is None or dereverb is False:
        return None
    import enhance
    if dereverb is True:
        dereverb = {}
    if not isinstance(dereverb, dict):
        raise ValueError(' - ERROR, {}: dereverb must be None, True or a dict of enhance.wpe_batch keywords, got {!r}'.format(
            what, dereverb))
    if 'return_taps' in dereverb:
        raise ValueError(' - ERROR, {}: dereverb: return_taps is not offered here (call enhance.dereverb_batch)'.format(what))
    hop = int(cfg_d['hop_length'])
    cfg, _ = enhance.check_wpe_keywords(what + ': dereverb', dereverb, hop, cfg_d['sample_rate'], int(cfg_d['win_length']))
    enhance._check_wpe_frames(what + ': dereverb', 1 + int(Lmax) // hop, cfg)
    return cfg


def _convert_host(what, decoder, wav, lens, cfg_d, t_s, t_e, two_pass, utt_ids, window_batch, vocode, encoder, wav_sr, out_sr,
                  res_type, denoise=None, dereverb=None, need_decoder=True):
    """The host checks and tables that convert_batch and convert_duration_batch share, before anything touches the GPU.
    need_decoder=False: the decoder-free entry point (convert_knn_diff_batch), which checks its own encoder / ppg pair.
    denoise, dereverb: the entry point's own arguments (_check_denoise, _check_dereverb); when either is on, every length is
    cut to whole hops first -- len' = hop * (len // hop), what the filter and the inverse transform return -- so under one
    hop is dropped and no frame count changes."""
    import audio_lib
    if getattr(wav, 'ndim', 0) != 2:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    n_fft = cfg_d['n_fft'] or cfg_d['win_length']
    h_lens = np.full((B,), Lmax, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    sr = cfg_d['sample_rate']
    audio_lib._res_params(res_type)
    res_in = wav_sr is not None and audio_lib._ratio(wav_sr, sr) != (1, 1)
    res_out = vocode and out_sr is not None and audio_lib._ratio(sr, out_sr) != (1, 1)
    h_lens_in = None
    if res_in:
        # lens count samples at wav_sr; everything below (checks, tables) works on the resampled lengths
        if h_lens.shape != (B,) or h_lens.min() <= 0 or h_lens.max() > Lmax:
            raise ValueError(' - ERROR, {}: lens must be [B] with 0 < len <= Lmax'.format(what))
        h_lens_in, Lmax_in = h_lens, Lmax
        h_lens, Lmax = audio_lib.resample_len(h_lens_in, wav_sr, sr), audio_lib.resample_len(Lmax_in, wav_sr, sr)
        if h_lens.min() <= n_fft // 2:
            raise ValueError(' - ERROR, {}: every utterance needs more than n_fft//2 = {} samples at {} Hz '
                             '(shortest: {} after resampling from {} Hz)'.format(what, n_fft // 2, sr, int(h_lens.min()), wav_sr))
    if h_lens.shape != (B,) or h_lens.min() <= n_fft // 2 or h_lens.max() > Lmax:
        raise ValueError(' - ERROR, {}: lens must be [B] with n_fft//2 < len <= Lmax'.format(what))
    denoise = _check_denoise(what, denoise, cfg_d, B)
    dereverb = _check_dereverb(what, dereverb, cfg_d, Lmax)
    if denoise is not None or dereverb is not None:
        h_lens = int(cfg_d['hop_length']) * (h_lens // int(cfg_d['hop_length']))
        if h_lens.min() <= n_fft // 2:
            raise ValueError(' - ERROR, {}: {}: every utterance needs more than n_fft//2 = {} samples after the cut to '
                             'whole hops (shortest: {})'.format(what, 'denoise' if denoise is not None else 'dereverb', n_fft // 2,
                                                                int(h_lens.min())))
    if utt_ids is None:
        utt_ids = np.arange(B)
    utt_ids = np.asarray(utt_ids, dtype=np.int64).reshape(-1)
    if utt_ids.shape != (B,) or utt_ids.min() < -2 ** 31 or utt_ids.max() >= 2 ** 31:
        raise ValueError(' - ERROR, {}: utt_ids must be {} int32 values, one per utterance'.format(what, B))
    window_batch = int(window_batch)
    if window_batch <= 0:
        raise ValueError(' - ERROR, {}: window_batch must be positive'.format(what))
    if need_decoder and (decoder.encoder is None) == (encoder is None):
        raise ValueError(' - ERROR, {}: pass encoder= exactly when the decoder was built without one'.format(what))
    plan = convert_plan(h_lens, cfg_d, t_s, t_e, two_pass)
    hop = int(cfg_d['hop_length'])
    if vocode and hop * (int(plan.n_out.min()) - 1) <= n_fft // 2:
        raise ValueError(' - ERROR, {}: every utterance needs hop_length*(frames-1) > n_fft//2 samples'.format(what))
    return _HOST_NT(plan, B, hop, n_fft, 1 + n_fft // 2, h_lens, h_lens_in, hop * (plan.n_out.astype(np.int64) - 1), utt_ids,
                    res_in, res_out, window_batch, denoise, dereverb)


def _convert_upload(h, wav, extra):
    """The waveforms if they are on the host, and one pinned table: the seven of the plan, the lengths at wav_sr when the
    input is resampled, then ``extra`` (host int arrays); d_extra holds the device views of those last ones in that order."""
    import torch
    plan = h.plan
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    parts = [h.h_lens, plan.n_clip, plan.n_out, h.utt_ids, plan.win_tab, plan.utt_tab, plan.true_tab]
    if h.res_in:
        parts.append(h.h_lens_in)
    parts += list(extra)
    h_tab = torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in parts])).pin_memory()
    d_tab = h_tab.to('cuda', non_blocking=True)
    offs = np.cumsum([0] + [a.size for a in parts])
    d_lens, d_clip, d_nout, d_ids, d_win, d_utt, d_true = (d_tab[offs[i]:offs[i + 1]] for i in range(7))
    d_extra = [d_tab[offs[i]:offs[i + 1]] for i in range(7, len(parts))]
    return _UP_NT(wav, d_lens, d_clip, d_nout, d_ids, d_win.view(-1, 2), d_utt.view(-1, 3), d_true.view(-1, 2), d_extra)


def _resample_input(h, up, cfg_d, wav_sr, res_type):
    """The input at the model's rate, resampled once: (h, up) with the waveform replaced and res_in cleared.  An entry point
    that reads up.wav itself (a tracker, the differential filter) calls this before _convert_model, which then finds
    nothing left to do."""
    import audio_lib
    if not h.res_in:
        return h, up
    wav = audio_lib._resample_launch(audio_lib._get_res_plan(wav_sr, cfg_d['sample_rate'], res_type), up.wav, up.d_extra[0])
    return h._replace(res_in=False), up._replace(wav=wav)


def _denoise_input(h, up, cfg_d, denoise):
    """The input with its stationary noise suppressed, once: (h, up) with the waveform replaced by enhance.denoise_batch's
    output and h.denoise cleared.  denoise: h.denoise, the checked request of _convert_host (None: nothing is launched).
    Runs right after _resample_input, at the model's rate; an entry point that reads up.wav itself (a tracker, the
    differential filter) calls this before _convert_model, which then finds nothing left to do.  The lengths were cut to
    whole hops on the host, so the filter's hop * (F - 1) samples are every utterance's whole length.
    h.dereverb (the checked request of _check_dereverb) is served here too, BEFORE the noise suppression and under the same
    rule: the waveform is replaced by enhance.dereverb_batch's output and h.dereverb cleared.  With both None nothing is
    launched."""
    import audio_lib
    import enhance
    if h.dereverb is not None:
        plan = audio_lib._get_voc_plan(cfg_d['win_length'], h.hop, cfg_d['n_fft'])
        r = enhance._dereverb_launch(plan, up.wav, up.d_lens, None, 1 + up.wav.shape[1] // h.hop, h.dereverb, False)
        h, up = h._replace(dereverb=None), up._replace(wav=r.y)
    if denoise is None:
        return h, up
    cfg, noise0 = denoise
    plan = audio_lib._get_voc_plan(cfg_d['win_length'], h.hop, cfg_d['n_fft'])
    r = enhance._denoise_launch(plan, up.wav, up.d_lens, None, 1 + up.wav.shape[1] // h.hop, cfg,
                                None if noise0 is None else enhance._as_cuda_f32(noise0), False)
    return h._replace(denoise=None), up._replace(wav=r.y)


def _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type):
    """Input resampling, noise suppression (h.denoise), front-end, windows and the model over window chunks: (mel_true,
    stft_true [B, Fout, C] and the window batches y_mel, y_stft, y_phn [W, T, C] that compound_stitch takes)."""
    import torch
    import audio_lib
    h, up = _resample_input(h, up, cfg_d, wav_sr, res_type)
    h, up = _denoise_input(h, up, cfg_d, h.denoise)
    plan, hop = h.plan, h.hop
    mfcc, mel, pdb = audio_lib.calc_MFCC_input_batch(
        up.wav, up.d_lens, sr=cfg_d['sample_rate'], pre_emphasis=cfg_d['pre_emphasis'], hop_length=hop,
        win_length=cfg_d['win_length'], n_mels=cfg_d['n_mels'], n_mfcc=cfg_d['n_mfcc'], n_fft=cfg_d['n_fft'],
        window=cfg_d['window'], mfcc_normaleze_first_mfcc=cfg_d['mfcc_normaleze_first_mfcc'],
        mfcc_norm_factor=cfg_d['mfcc_norm_factor'], calc_mfcc_derivate=cfg_d['calc_mfcc_derivate'],
        M_dB_norm_factor=cfg_d['M_dB_norm_factor'], P_dB_norm_factor=cfg_d['P_dB_norm_factor'],
        mean_abs_amp_norm=cfg_d['mean_abs_amp_norm'], clip_output=cfg_d['clip_output'])
    x = cut_windows(mfcc, up.d_win, up.d_clip, plan.T)
    mel_true = cut_windows(mel, up.d_true, up.d_clip, plan.Fout)
    stft_true = cut_windows(pdb, up.d_true, up.d_clip, plan.Fout)
    if encoder is None:
        outs = decoder.forward_chunks(x, h.window_batch, n_streams=2)
    else:
        outs = decoder.forward_chunks(x, h.window_batch, n_streams=2, width=x.shape[2],
                                      fn=lambda xb: decoder.forward(encoder.forward(xb)['y_pred']))
    main = torch.cuda.current_stream()
    cols = []
    for key in ('y_mel', 'y_stft', 'y_phn'):
        ts = [o[key] for o in outs]
        for t in ts:
            t.record_stream(main)
        cols.append(ts[0] if len(ts) == 1 else torch.cat(ts, 0))
    return (mel_true, stft_true) + tuple(cols)


def _vocoder_tail(cfg_d, d_nf, d_ids, n_iter, momentum, realse, seed, ph_true, ph_pred, stft_true, stft_pred, amp_pred):
    """The vocoder behind a conversion, on frame counts that only the device needs to know (d_nf int32 [B]): the phase
    start, the magnitudes, Griffin-Lim, de-emphasis and level.  stft_pred [B, F, bins]; amp_pred: its magnitude where a
    kernel before this already made it (realse == 1), else None (made here); stft_true: None, or the true
    spectrum to vocode as well.  ph_*: 'device' (one vc_phase_init from seed and d_ids, shared by both spectra), 'spsi' (from
    each spectrum's own magnitudes) or a [B, F, bins] tensor.  Returns (y_wav_true | None, y_wav_pred) at the model's rate."""
    import audio_lib
    _, F, n_bins = stft_pred.shape
    vplan = audio_lib._get_voc_plan(cfg_d['win_length'], int(cfg_d['hop_length']), cfg_d['n_fft'])
    if isinstance(ph_pred, str) and ph_pred == 'device':
        ph_true = ph_pred = audio_lib.phase_init(d_nf, F, n_bins, seed, d_ids)
    elif isinstance(ph_pred, str):
        ph_true = ph_pred = None                                   # 'spsi': from each spectrum's own magnitudes, in to_wav

    def to_wav(amp, ph):
        if ph is None:
            ph = audio_lib._phase_spsi_launch(amp, d_nf, vplan.n_fft, vplan.hop_length, plan=vplan)
        w = audio_lib._griffin_lim_launch(vplan, amp, ph, d_nf, n_iter, False, momentum)
        return _deemphasis_level(vplan, w, d_nf, F, cfg_d, cfg_d['pre_emphasis'])

    y_wav_true = to_wav(_power_to_amp(stft_true, d_nf, cfg_d, 1.0), ph_true) if stft_true is not None else None
    y_wav_pred = to_wav(amp_pred if amp_pred is not None else _power_to_amp(stft_pred, d_nf, cfg_d, realse), ph_pred)
    return y_wav_true, y_wav_pred


def _power_to_amp(P, d_nf, cfg_d, realse):
    """The vocoder's magnitude of the spectrum P [B, F, bins] over d_nf frames per utterance."""
    import torch
    import _vc
    B, F, n_bins = P.shape
    amp = torch.empty_like(P)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(P), _vc.ptr(d_nf), B, F, n_bins, float(cfg_d['P_dB_norm_factor']), float(realse),
                                        _vc.ptr(amp), _vc.current_stream()))
    return amp


def _deemphasis_level(vplan, w, d_nf, F, cfg_d, pre_emphasis):
    """In place: the waveforms w [B, L] of d_nf frames (of at most F) de-emphasised and
    brought to the level 15 * mean_abs_amp_norm.  pre_emphasis 0.0 sets the level alone.  Returns w."""
    import _vc
    _vc.check(_vc.lib().vc_inv_preemphasis_normalize(vplan.handle, _vc.ptr(w), _vc.ptr(d_nf), w.shape[0], F, w.shape[1],
                                                     float(pre_emphasis), float(15 * cfg_d['mean_abs_amp_norm']),
                                                     _vc.current_stream()))
    return w


def _stitch(y_mel, y_phn, y_stft, d_utt, Fout, P_dB_norm_factor=None):
    """The three window batches of _convert_model stitched, launched in this order: (mel, phn, stft, amp).  With
    P_dB_norm_factor the spectrum's launch writes the vocoder's magnitude as well (realse == 1); amp is None without."""
    mel = compound_stitch(y_mel, d_utt, Fout)
    phn = compound_stitch(y_phn, d_utt, Fout)
    if P_dB_norm_factor is None:
        return mel, phn, compound_stitch(y_stft, d_utt, Fout), None
    return (mel, phn) + compound_stitch(y_stft, d_utt, Fout, P_dB_norm_factor=P_dB_norm_factor)


def _resample_output(y, h_nsamp, d_nsamp, res_out, cfg_d, out_sr, res_type):
    """The output tail on host-known sample counts: (y resampled to out_sr when res_out, n_samples as a host list at the rate
    returned).  d_nsamp: h_nsamp on the device, read only when res_out."""
    import audio_lib
    if not res_out:
        return y, [int(v) for v in h_nsamp]
    sr = cfg_d['sample_rate']
    y = audio_lib._resample_launch(audio_lib._get_res_plan(sr, out_sr, res_type), y, d_nsamp)
    return y, [int(v) for v in audio_lib.resample_len(h_nsamp, sr, out_sr)]


def convert_batch(decoder, wav, lens=None, cfg_d=None, t_s=0, t_e=60, n_iter=200, realse=1.0, two_pass=True,
                  giffin_lim_input=False, momentum=0.0, phase='device', seed=0, utt_ids=None, window_batch=64,
                  vocode=True, encoder=None, wav_sr=None, out_sr=None, res_type='kaiser_best', denoise=None,
                  dereverb=None):
    """``conversion2`` (two_pass) / ``conversion`` for a ragged batch, waveforms in, waveforms out, on the device.

    wav [B, Lmax] float32 (numpy or cuda tensor), lens: host ints (None = all Lmax).  cfg_d: the data-set
    configuration of test.py (sample_rate, hop_length, win_length, n_fft, n_timesteps, the front-end's settings).
    phase: 'device' (vc_phase_init from ``seed`` and ``utt_ids``, default 0 .. B-1; the true and the predicted
    spectrum start from the same phase), 'numpy' (the reference's draws from the global generator, in the order of a
    loop of conversion2 calls), 'spsi' (audio_lib.phase_spsi: computed from the magnitudes, so the true and the predicted
    spectrum each get the start of their own; ``seed`` and ``utt_ids`` are ignored) or a [B, Fout, bins] array.
    window_batch: windows per decoder chunk (utterances and passes mixed), issued round-robin on the decoder's streams.
    vocode=False stops after the stitch.
    encoder: only for a decoder built WITHOUT one (an MX-FP8 decoder owns its store and takes posteriors): the
    encoder whose posteriors feed it, chunk by chunk on the same streams.
    wav_sr: the sample rate of ``wav`` (None = cfg_d['sample_rate']); another rate is resampled on the device first
    (audio_lib.resample_batch, ``res_type``), and ``lens`` then count samples at wav_sr.  out_sr: the rate of the returned
    waveforms (None = cfg_d['sample_rate']); n_samples is then reported at out_sr.
    dereverb: None / False (today's launches and nothing else), True (enhance.dereverb_batch at the defaults of the data
    set's framing) or a dict of enhance.wpe_batch's keywords: late reverberation is taken out of the input once, at the
    model's rate and BEFORE the noise suppression, under denoise's rule (lengths cut to whole hops first).
    denoise: None / False (today's launches and nothing else), True (enhance.denoise_batch at its defaults) or a dict of its
    noise-suppression keywords: stationary noise is taken out of the input at the model's rate, right after the input
    resampler, before anything reads the waveform.  Every utterance is first cut to whole hops (under one hop is dropped, no
    frame count changes); mel_true / stft_true are then those of the DENOISED input.
    Returns a namedtuple of cuda tensors -- y_wav_pred, y_wav_true (None unless giffin_lim_input) [B, hop*(Fout-1)],
    mel_pred / stft_pred / phn_pred and mel_true / stft_true [B, Fout, C], zero beyond an utterance's own extent --
    and the host counts n_frames [B] (= N_b * n_timesteps) and n_samples [B] (= hop * (n_frames - 1)).
    Every check and every table is made on the host from ``lens`` before the first launch; after that nothing is
    copied to the host and the host waits for nothing."""
    import torch
    import audio_lib
    what = 'convert_batch'
    momentum = _check_momentum(momentum)
    seed = audio_lib.check_seed(seed)
    _need_cfg(cfg_d, what)
    _check_phase(phase, what, None, ('device', 'numpy', 'spsi'))
    h = _convert_host(what, decoder, wav, lens, cfg_d, t_s, t_e, two_pass, utt_ids, window_batch, vocode, encoder, wav_sr, out_sr,
                      res_type, denoise, dereverb)
    plan, Fout, n_bins = h.plan, h.plan.Fout, h.n_bins
    both = bool(giffin_lim_input)
    _check_phase(phase, what, (h.B, Fout, n_bins), ('device', 'numpy', 'spsi'))
    _need_gpu(what)

    # ---- uploads: the waveforms if they are on the host, one table, the host-drawn phase if asked for
    up = _convert_upload(h, wav, [h.h_nsamp] if h.res_out else [])
    ph_true = ph_pred = phase                                      # 'device' / 'spsi': made in the vocoder tail
    if vocode and isinstance(phase, str) and phase == 'numpy':
        d_phase = torch.from_numpy(_numpy_phase(plan, n_bins, both)).pin_memory().to('cuda', non_blocking=True)
        ph_true, ph_pred = d_phase[0], d_phase[-1]
    elif vocode:
        ph_true = ph_pred = _phase_upload(phase)

    # ---- front-end, windows, model, stitch
    mel_true, stft_true, y_mel, y_stft, y_phn = _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type)
    fused = vocode and float(realse) == 1.0
    mel_pred, phn_pred, stft_pred, amp_pred = _stitch(y_mel, y_phn, y_stft, up.d_utt, Fout,
                                                      cfg_d['P_dB_norm_factor'] if fused else None)

    # ---- vocoder, output rate
    y_wav_true = y_wav_pred = None
    if vocode:
        y_wav_true, y_wav_pred = _vocoder_tail(cfg_d, up.d_nout, up.d_ids, n_iter, momentum, realse, seed, ph_true, ph_pred,
                                               stft_true if both else None, stft_pred, amp_pred)
    d_nsamp = up.d_extra[-1] if h.res_out else None
    y_wav_pred, n_samples = _resample_output(y_wav_pred, h.h_nsamp, d_nsamp, h.res_out, cfg_d, out_sr, res_type)
    if both:
        y_wav_true, _ = _resample_output(y_wav_true, h.h_nsamp, d_nsamp, h.res_out, cfg_d, out_sr, res_type)
    return _BATCH_NT(y_wav_true, y_wav_pred, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred,
                     [int(v) for v in plan.n_out])


# --------------------------------------------------------------------------- duration (csrc/vc_warp.hip)
WARP_MAX_FRAMES = 16384     # vc_duration_map, vc_time_warp: input frames, output frames, table entries
WARP_MAX_RATIO = 8.0
WARP_Q = 65536
FLAG_INVALID, FLAG_SHORT, FLAG_TRUNCATED = 1, 2, 4
_MAP_NT = namedtuple('duration_map', 'pos n_out out_start out_end flags max_frames')
_STATS_NT = namedtuple('duration_stats', 'count total')
_DUR_NT = namedtuple('convert_duration', 'y_wav_pred n_samples mel_pred stft_pred phn_pred n_frames flags seg map max_frames '
                                         'max_samples src_frames')
_DUR_SEG_NT = namedtuple('duration_segments', 'labels start end n_seg')


def _i32_device(a, shape, what):
    """int32 of the given shape on the device: a cuda tensor is checked and used as it is, a host array goes up pinned."""
    import torch
    if torch.is_tensor(a) and a.is_cuda:
        if a.dtype != torch.int32 or tuple(a.shape) != tuple(shape):
            raise ValueError(' - ERROR, {} on the device must be int32 {}, got {} {}'.format(what, list(shape), a.dtype, list(a.shape)))
        return a.contiguous()
    h = np.asarray(a.cpu() if torch.is_tensor(a) else a)
    if h.shape != tuple(shape) or h.dtype.kind not in 'iu' or (h.size and (h.min() < -2 ** 31 or h.max() >= 2 ** 31)):
        raise ValueError(' - ERROR, {} must be integers of shape {}'.format(what, list(shape)))
    return torch.from_numpy(np.ascontiguousarray(h, dtype=np.int32)).pin_memory().to('cuda', non_blocking=True)


def ratio_to_q(ratio):
    """Q16 rates as the launch takes them: float32, times 65,536 (exact), rounded to the nearest integer with ties to even,
    clamped to [0, 8 * 65,536].  A host array gives a numpy int32 array, a tensor an int32 tensor on its device."""
    import torch
    if torch.is_tensor(ratio):
        return torch.round(ratio.to(torch.float32) * float(WARP_Q)).clamp(0, WARP_MAX_RATIO * WARP_Q).to(torch.int32)
    r = np.rint(np.asarray(ratio, dtype=np.float32) * np.float32(WARP_Q))
    return np.clip(r, 0, WARP_MAX_RATIO * WARP_Q).astype(np.int32)


def _check_ratio_scalar(r, what):
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not 0.0 <= float(r) <= WARP_MAX_RATIO:
        raise ValueError(' - ERROR, {} must be a number in [0, {}], got {!r}'.format(what, WARP_MAX_RATIO, r))
    return int(ratio_to_q(float(r)))


def duration_max_frames(n_max, n_pieces, ratio_max_q):
    """The default output bound of duration_map_batch in rate mode (host integers): see the proof there."""
    n_max, p = int(n_max), min(int(n_pieces), int(n_max))
    return max(n_max, (n_max * int(ratio_max_q) + WARP_Q - 1) // WARP_Q + (p + 1) // 2)


def duration_map_batch(start, end, n_seg, lens, out_len=None, labels=None, ratio=None, gap_ratio=1.0, max_frames=None,
                       min_frames=1):
    """The integer time map of B utterances from their segment tables (vc_duration_map; the definition is in
    include/vc_hip.h, "Duration", the numpy restatement in tests/warp_ref.py).

    start, end [B, K] int32 (end exclusive) and n_seg [B]: a segment table in frames as phn_segments_batch, align_batch and
    decode_batch return it (device tensors or host arrays; an entry with start < 0 or end == start is absent).  lens: the
    frame counts n, host integers or an int32 [B] device tensor.  One of
      out_len [B, K] int32   the output length of every present segment (0 deletes it),
      ratio                  floats [C] indexed by labels [B, K] (or one number for every segment, without labels): the
                             segment gets round(Li * ratio) frames; rounded to Q16 on the device when it is a device tensor,
      neither                segments keep their length.
    gap_ratio: the rate of the frames outside the segments.  Rates lie in [0, 8].  min_frames: an utterance whose total
    would fall below it keeps the identity map (flag 2).  max_frames: the host-known bound Fw_max of the output; an
    utterance that exceeds it is cut there (flag 4).

    The default max_frames (rate mode, host lens) cannot truncate.  Proof: the pieces' input lengths Li add up to n, a
    piece of Li == 0 gets Lo == 0, and a piece of Li > 0 gets Lo = (Li * q + 32768) >> 16 <= Li * q / 65536 + 1/2 with
    q <= q_max, the largest Q16 rate in play (ratio's maximum and gap_ratio; 8 * 65536 for a ratio that lives on the
    device).  There are at most P = min(2 K + 1, n) pieces of Li > 0, so the total is at most n * q_max / 65536 + P / 2, and
    being an integer at most ceil(n * q_max / 65536) + ceil(P / 2) -- the default, taken at the longest utterance (it grows
    with n), raised to n_max itself for the identity map of flags 1 and 2, and capped at the launch's limit of 16,384 (only
    then can flag 4 appear).  With out_len, or with lens on the device, the bound is not derivable: pass max_frames.

    Returns a namedtuple of device tensors: pos [B, max_frames] int32 (Q16 input frames, -1 from n_out on), n_out [B],
    out_start / out_end [B, K] (the table in output frames), flags [B] (1 invalid table, 2 below min_frames: identity map;
    4 truncated) and the host integer max_frames.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'duration_map_batch'
    if getattr(start, 'ndim', 0) != 2 or start.shape[1] < 1 or start.shape[0] < 1:
        raise ValueError(' - ERROR, {}: start must be [B, K] with B, K >= 1'.format(what))
    B, K = int(start.shape[0]), int(start.shape[1])
    if out_len is not None and (ratio is not None or labels is not None):
        raise ValueError(' - ERROR, {}: out_len excludes ratio and labels'.format(what))
    if labels is not None and ratio is None:
        raise ValueError(' - ERROR, {}: labels index ratio; pass both'.format(what))
    if B > 65535 or K > WARP_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most {} table entries'.format(what, WARP_MAX_FRAMES))
    gap_q = _check_ratio_scalar(gap_ratio, what + ': gap_ratio')
    if isinstance(min_frames, bool) or not isinstance(min_frames, (int, np.integer)) or not 0 <= min_frames <= WARP_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: min_frames must be an integer in [0, {}]'.format(what, WARP_MAX_FRAMES))
    lens_dev = torch.is_tensor(lens) and lens.is_cuda
    n_max = None
    if not lens_dev:
        h_lens = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens)
        if h_lens.shape != (B,) or h_lens.dtype.kind not in 'iu' or h_lens.min() < 0 or h_lens.max() > WARP_MAX_FRAMES:
            raise ValueError(' - ERROR, {}: lens must be {} integers in [0, {}]'.format(what, B, WARP_MAX_FRAMES))
        n_max = int(h_lens.max())
    q_max = gap_q
    if ratio is not None:
        if not torch.is_tensor(ratio):
            ratio = np.atleast_1d(np.asarray(ratio, dtype=np.float32))
            if ratio.ndim != 1 or not np.isfinite(ratio).all() or ratio.min() < 0 or ratio.max() > WARP_MAX_RATIO:
                raise ValueError(' - ERROR, {}: ratio must be finite floats [C] in [0, {}]'.format(what, WARP_MAX_RATIO))
            q_max = max(q_max, int(ratio_to_q(ratio).max()))
        else:
            if ratio.ndim != 1 or not ratio.is_floating_point():
                raise ValueError(' - ERROR, {}: ratio must be floats [C]'.format(what))
            q_max = int(WARP_MAX_RATIO * WARP_Q)
        if ratio.shape[0] < 1 or (labels is None and ratio.shape[0] != 1):
            raise ValueError(' - ERROR, {}: without labels ratio is one number; with labels it is [C], C >= 1'.format(what))
    if max_frames is None:
        if out_len is not None or n_max is None:
            raise ValueError(' - ERROR, {}: max_frames is required with out_len and with lens on the device'.format(what))
        max_frames = min(max(duration_max_frames(n_max, 2 * K + 1, q_max), 1), WARP_MAX_FRAMES)
    if isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer)) or not 1 <= max_frames <= WARP_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: max_frames must be an integer in [1, {}]'.format(what, WARP_MAX_FRAMES))
    _need_gpu(what)
    d_start, d_end = _i32_device(start, (B, K), what + ': start'), _i32_device(end, (B, K), what + ': end')
    d_nseg, d_lens = _i32_device(n_seg, (B,), what + ': n_seg'), _i32_device(lens, (B,), what + ': lens')
    d_len = None if out_len is None else _i32_device(out_len, (B, K), what + ': out_len')
    d_lab = None if labels is None else _i32_device(labels, (B, K), what + ': labels')
    d_ratio = None
    if ratio is not None:
        if torch.is_tensor(ratio):
            d_ratio = ratio_to_q(ratio.to('cuda', non_blocking=True)).contiguous()
        else:
            d_ratio = _i32_device(ratio_to_q(ratio), ratio.shape, what + ': ratio')
    return _map_launch(d_start, d_end, d_nseg, d_lab, d_len, d_ratio, gap_q, d_lens, WARP_MAX_FRAMES if n_max is None else max(n_max, 1),
                       int(min_frames), int(max_frames))


def _map_launch(d_start, d_end, d_nseg, d_lab, d_len, d_ratio, gap_q, d_lens, in_frames, min_frames, Fw):
    """vc_duration_map on validated device tensors: no host check, copy or wait in here."""
    import torch
    import _vc
    lib = _vc.lib()
    B, K = d_start.shape
    dev = d_start.device
    pos = torch.empty((B, Fw), dtype=torch.int32, device=dev)
    tab = torch.empty((2, B, K), dtype=torch.int32, device=dev)
    small = torch.empty((2, B), dtype=torch.int32, device=dev)
    need = lib.vc_duration_map_workspace_bytes(B, K)
    if need == 0:
        raise _vc.VCError('vc_duration_map_workspace_bytes refused {} utterances of {} table entries'.format(B, K))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    _vc.check(lib.vc_duration_map(_vc.ptr(d_start), _vc.ptr(d_end), _vc.ptr(d_nseg), _vc.ptr(d_lab), _vc.ptr(d_len), _vc.ptr(d_ratio),
                                  0 if d_ratio is None else d_ratio.shape[0], gap_q, _vc.ptr(d_lens), B, K, in_frames, min_frames, Fw,
                                  _vc.ptr(pos), _vc.ptr(small[0]), _vc.ptr(tab[0]), _vc.ptr(tab[1]), _vc.ptr(small[1]), _vc.ptr(ws),
                                  need, _vc.current_stream()))
    return _MAP_NT(pos, small[0], tab[0], tab[1], small[1], Fw)


def _warp_launch(x, pos, n_out, d_lens, mode, P_dB_norm_factor=None):
    """vc_time_warp on validated device tensors; with P_dB_norm_factor also the vocoder's magnitude: (warped, amp)."""
    import torch
    import _vc
    B, F, C = x.shape
    Fw = pos.shape[1]
    out = torch.empty((B, Fw, C), dtype=torch.float32, device=x.device)
    amp = torch.empty_like(out) if P_dB_norm_factor is not None else None
    _vc.check(_vc.lib().vc_time_warp(_vc.ptr(x), _vc.ptr(pos), _vc.ptr(n_out), _vc.ptr(d_lens), B, F, Fw, C, mode, _vc.ptr(out),
                                     _vc.ptr(amp), float(P_dB_norm_factor or 0.0), _vc.current_stream()))
    return out if P_dB_norm_factor is None else (out, amp)


_WARP_MODES = {'linear': 0, 'nearest': 1}                           # VC_WARP_LINEAR, VC_WARP_NEAREST


def time_warp_batch(x, pos, n_out, lens, mode='linear', P_dB_norm_factor=None):
    """Resamples x [B, F, C] float32 (cuda tensor or numpy array) along a time map (vc_time_warp): pos [B, Fw] int32 Q16
    input frames and n_out [B], device tensors as duration_map_batch returns them; lens: the input frame counts, host
    integers, an int32 [B] device tensor or None (all F).  mode 'linear': row u is a + w * (b - a) of the two input rows
    around pos[u] (three float32 roundings; the row itself where pos[u] is a whole frame), 'nearest': the nearest row.
    Rows from n_out on are zero.  With P_dB_norm_factor also the vocoder's magnitude of the warped spectrum (what
    vc_power_to_amp gives with realse == 1, bit for bit): returns (warped, amp).  Nothing is copied back."""
    import torch
    what = 'time_warp_batch'
    if mode not in _WARP_MODES:
        raise ValueError(" - ERROR, {}: mode must be 'linear' or 'nearest', got {!r}".format(what, mode))
    if getattr(x, 'ndim', 0) != 3 or min(x.shape) < 1:
        raise ValueError(' - ERROR, {}: x must be [B, F, C]'.format(what))
    B, F, C = (int(v) for v in x.shape)
    if not (torch.is_tensor(pos) and pos.is_cuda and pos.dtype == torch.int32 and pos.ndim == 2 and pos.shape[0] == B and pos.shape[1] >= 1):
        raise ValueError(' - ERROR, {}: pos must be an int32 [B, Fw] device tensor'.format(what))
    Fw = int(pos.shape[1])
    if B > 65535 or F > WARP_MAX_FRAMES or Fw > WARP_MAX_FRAMES or max(F, Fw) * C >= 2 ** 30:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most {} frames in and out, frames * C < 2^30'.format(what, WARP_MAX_FRAMES))
    if P_dB_norm_factor is not None and float(P_dB_norm_factor) == 0.0:
        raise ValueError(' - ERROR, {}: P_dB_norm_factor is 0'.format(what))
    if lens is not None and not (torch.is_tensor(lens) and lens.is_cuda):
        h = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > F:
            raise ValueError(' - ERROR, {}: lens must be {} integers in [0, {}]'.format(what, B, F))
    _need_gpu(what)
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = x.to(device='cuda', dtype=torch.float32).contiguous()
    d_lens = None if lens is None else _i32_device(lens, (B,), what + ': lens')
    return _warp_launch(x, pos.contiguous(), _i32_device(n_out, (B,), what + ': n_out'), d_lens, _WARP_MODES[mode], P_dB_norm_factor)


def duration_stats_batch(labels, start, end, n_seg, n_classes):
    """Per-class segment count and total length (frames) over a batch of segment tables, as align_batch / decode_batch
    return them: (count [C], total [C]) int64 tensors on the tables' device.  Entries from n_seg on, absent entries
    (start < 0 or end <= start) and labels outside [0, C) are left out.  Plain torch (index_add_): no kernel of this
    library, nothing copied back."""
    import torch
    labels, start, end, n_seg = (torch.as_tensor(t) for t in (labels, start, end, n_seg))
    C = int(n_classes)
    K = labels.shape[-1]
    k = torch.arange(K, device=labels.device)
    keep = (k[None, :] < n_seg.reshape(-1, 1)) & (start >= 0) & (end > start) & (labels >= 0) & (labels < C)
    idx = labels.clamp(0, C - 1).reshape(-1).long()
    count = torch.zeros((C,), dtype=torch.int64, device=labels.device).index_add_(0, idx, keep.reshape(-1).long())
    total = torch.zeros((C,), dtype=torch.int64, device=labels.device).index_add_(0, idx, ((end - start) * keep).reshape(-1).long())
    return _STATS_NT(count, total)


def duration_ratios(stats_src, stats_tgt, lo=0.5, hi=2.0, min_count=1):
    """The rate table that gives the source's phonemes the target's mean durations: per class
    clamp(mean_tgt / mean_src, lo, hi) with mean = total / count of duration_stats_batch, and 1 where either side has
    fewer than ``min_count`` segments (or no frames).  float32 [C] on the statistics' device; no synchronisation."""
    import torch
    if not 0.0 <= float(lo) <= float(hi) <= WARP_MAX_RATIO:
        raise ValueError(' - ERROR, duration_ratios: need 0 <= lo <= hi <= {}'.format(WARP_MAX_RATIO))
    cs, ts, ct, tt = (torch.as_tensor(t) for t in (stats_src[0], stats_src[1], stats_tgt[0], stats_tgt[1]))
    mc = max(int(min_count), 1)
    ok = (cs >= mc) & (ct >= mc) & (ts > 0) & (tt > 0)
    one = torch.ones_like(ts, dtype=torch.float64)
    num = torch.where(ok, tt.double() * cs.double(), one)
    den = torch.where(ok, ts.double() * ct.double(), one)
    return torch.where(ok, (num / den).clamp(float(lo), float(hi)), one).to(torch.float32)


def duration_min_frames(cfg_d):
    """The fewest frames the vocoder takes: hop * (frames - 1) > n_fft // 2."""
    n_fft = cfg_d['n_fft'] or cfg_d['win_length']
    return (n_fft // 2) // int(cfg_d['hop_length']) + 2


_DUR_REQ_NT = namedtuple('duration_request', 'rate rate_q ratio out_len gap_q table decode K Fw min_frames dec cmap')


def _duration_request(what, rate, ratio, gap_ratio, segments, decode, out_len):
    """The duration arguments of convert_duration_batch and convert_diff_duration_batch, as far as they can be checked
    without a plan: rate_q / gap_q (Q16), table (the caller's segment table, None for rate= and for 'decode') and decode (the
    phone-loop decoder's keywords with their defaults).  K, Fw, min_frames come from _duration_bound, dec and cmap from
    _duration_decoder."""
    if sum(v is not None for v in (rate, ratio, out_len)) != 1:
        raise ValueError(' - ERROR, {}: pass exactly one of rate, ratio and out_len'.format(what))
    rate_q = None
    if rate is not None:
        if isinstance(rate, bool) or not isinstance(rate, (int, float, np.integer, np.floating)) or not 0.0 < float(rate) <= WARP_MAX_RATIO:
            raise ValueError(' - ERROR, {}: rate must be a number in (0, {}], got {!r}'.format(what, WARP_MAX_RATIO, rate))
        rate_q = int(ratio_to_q(float(rate)))
    gap_q = _check_ratio_scalar(gap_ratio, what + ': gap_ratio')
    table = None
    if rate is None and not (isinstance(segments, str) and segments == 'decode'):
        if isinstance(segments, str) or len(segments) != 4:
            raise ValueError(" - ERROR, {}: segments must be 'decode' or (labels, start, end, n_seg)".format(what))
        table = segments
    if decode is not None and (rate is not None or table is not None):
        raise ValueError(" - ERROR, {}: decode is for segments='decode'".format(what))
    kw = dict(trans=None, penalty=0.0, init=None, final=None, min_dur=3, class_map=None, floor=1e-10)
    extra = set(decode or {}) - set(kw)
    if extra:
        raise ValueError(' - ERROR, {}: decode takes {}, got {}'.format(what, sorted(kw), sorted(extra)))
    kw.update(decode or {})
    return _DUR_REQ_NT(rate, rate_q, ratio, out_len, gap_q, table, kw, None, None, None, None, None)


def _duration_bound(what, req, n_frames, Fout, min_frames, max_frames, needs):
    """After _convert_host: the table width K and the output bound Fw (max_frames, or its default where one can be derived)
    for utterances of n_frames (int64 [B], at most Fout) input frames.  min_frames: the fewest frames an output may have;
    needs: how the error of a rate= that falls below it ends."""
    import torch
    rate, ratio, table = req.rate, req.ratio, req.table
    if Fout > WARP_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: at most {} stitched frames per utterance (got {})'.format(what, WARP_MAX_FRAMES, Fout))
    K = 1 if rate is not None else (Fout if table is None else int(table[1].shape[1]))
    if rate is not None:
        want = (n_frames * req.rate_q + 32768) >> 16
        if want.min() < min_frames:
            raise ValueError(' - ERROR, {}: rate {} leaves an utterance {} frames; {}'.format(what, rate, int(want.min()),
                                                                                              needs.format(min_frames)))
        bound = int(want.max())
    elif ratio is not None and not torch.is_tensor(ratio):
        r = np.atleast_1d(np.asarray(ratio, dtype=np.float32))
        if r.ndim != 1 or not np.isfinite(r).all() or r.min() < 0 or r.max() > WARP_MAX_RATIO:
            raise ValueError(' - ERROR, {}: ratio must be finite floats [C] in [0, {}]'.format(what, WARP_MAX_RATIO))
        ratio = r
        bound = duration_max_frames(Fout, 2 * K + 1, max(req.gap_q, int(ratio_to_q(r).max())))
    else:
        if ratio is not None and (ratio.ndim != 1 or not ratio.is_floating_point()):
            raise ValueError(' - ERROR, {}: ratio must be floats [C]'.format(what))
        bound = None
    if max_frames is None:
        if bound is None:
            raise ValueError(' - ERROR, {}: max_frames is required with out_len and with a ratio on the device'.format(what))
        max_frames = min(bound, WARP_MAX_FRAMES)
    if isinstance(max_frames, bool) or not isinstance(max_frames, (int, np.integer)) or not min_frames <= max_frames <= WARP_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: max_frames must be an integer in [{}, {}]'.format(what, min_frames, WARP_MAX_FRAMES))
    return req._replace(ratio=ratio, K=K, Fw=int(max_frames), min_frames=min_frames)


def _duration_decoder(what, req, decoder, encoder, B, Fout):
    """The last host check of a duration request: with segments='decode', the phone-loop decoder's arguments (dec, cmap),
    before anything is launched."""
    if req.rate is not None or req.table is not None:
        return req
    import evaluation
    kw = dict(req.decode)
    C = int((encoder if encoder is not None else decoder.encoder).cfg_d['n_output'])
    evaluation._check_decode_size(B, Fout, C, what)
    cmap = evaluation._check_class_map(kw.pop('class_map'), C, what)
    return req._replace(dec=evaluation._decode_args(C=C, what=what, kind='prob', **kw), cmap=cmap)


def _duration_map(what, req, d_nf, phn, Fout):
    """The device side of a duration request: the segment table in input frames -- one piece per utterance for rate=, decoded
    from the posteriors phn [B, Fout, C] over d_nf [B] frames, or the caller's table -- and vc_duration_map over it.  Returns
    (map, seg): duration_map_batch's result and (labels, start, end, n_seg) in OUTPUT frames."""
    import torch
    B, K, dev = d_nf.shape[0], req.K, d_nf.device
    d_lab = d_len = d_ratio = None
    if req.rate is not None:
        d_start = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        d_end, d_nseg = d_nf.view(B, 1), torch.ones((B,), dtype=torch.int32, device=dev)
        d_ratio = torch.full((1,), req.rate_q, dtype=torch.int32, device=dev)
    else:
        if req.table is None:
            import evaluation
            r = evaluation._decode_launch(phn, d_nf, evaluation._cmap_device(req.cmap), evaluation._decode_upload(req.dec))
            d_lab, d_start, d_end, d_nseg = r.seg.labels, r.seg.start, r.seg.end, r.seg.n_seg
        else:
            d_lab, d_start, d_end = (_i32_device(t, (B, K), what + ': segments') for t in req.table[:3])
            d_nseg = _i32_device(req.table[3], (B,), what + ': segments n_seg')
        if req.out_len is not None:
            d_len = _i32_device(req.out_len, (B, K), what + ': out_len')
        elif torch.is_tensor(req.ratio):
            d_ratio = ratio_to_q(req.ratio.to('cuda', non_blocking=True)).contiguous()
        else:
            d_ratio = _i32_device(ratio_to_q(req.ratio), req.ratio.shape, what + ': ratio')
    m = _map_launch(d_start, d_end, d_nseg, None if d_ratio is None or req.rate is not None else d_lab, d_len, d_ratio, req.gap_q,
                    d_nf, Fout, req.min_frames, req.Fw)
    return m, _DUR_SEG_NT(d_lab, m.out_start, m.out_end, d_nseg)


def _resample_output_device(y, n_samples, max_samples, res_out, cfg_d, out_sr, res_type):
    """The output tail on sample counts that only the device knows (n_samples int32 [B], at most the host's max_samples):
    (y, n_samples, max_samples), at out_sr when res_out."""
    import torch
    import audio_lib
    if not res_out:
        return y, n_samples, max_samples
    sr = cfg_d['sample_rate']
    rplan = audio_lib._get_res_plan(sr, out_sr, res_type)
    y = audio_lib._resample_launch(rplan, y, n_samples)
    n_samples = torch.div(n_samples.long() * rplan.up + (rplan.down - 1), rplan.down, rounding_mode='floor').to(torch.int32)
    return y, n_samples, int(audio_lib.resample_len(max_samples, sr, out_sr))


def convert_duration_batch(decoder, wav, lens=None, cfg_d=None, rate=None, ratio=None, gap_ratio=1.0, segments='decode',
                           decode=None, out_len=None, max_frames=None, mode='linear', t_s=0, t_e=60, n_iter=200, realse=1.0,
                           two_pass=True, momentum=0.0, phase='device', seed=0, utt_ids=None, window_batch=64, encoder=None,
                           wav_sr=None, out_sr=None, res_type='kaiser_best', denoise=None,
                           dereverb=None):
    """``convert_batch`` with the timing changed as well: the stitched spectra are resampled along an integer time map
    (duration_map_batch, time_warp_batch) before the vocoder, which rebuilds the phase for the new timing.

    One of
      rate=r            every utterance as one piece: round(frames * r) output frames (0 < r <= 8); needs no segments;
      ratio=[C floats]  a rate per phoneme class (duration_ratios builds one from two speakers' alignments), gap_ratio for
                        the frames outside the segments;
      out_len [B, K]    an explicit length per segment.
    segments (ratio / out_len): 'decode' -- decode_batch on the stitched posteriors ``phn_pred`` (probabilities: kind='prob';
    ``decode``: a dict of its other arguments, e.g. trans, penalty, min_dur, class_map) -- or a table (labels, start, end,
    n_seg) in stitched-frame coordinates, e.g. from align_batch.  The other arguments are convert_batch's; phase='numpy'
    draws per host-known length and is refused here; denoise: the input denoised first, mel / stft of the denoised input.
    max_frames: the bound of the output frames (default: exact for
    rate=, duration_map_batch's proven bound for a host ratio, required otherwise).

    Every utterance keeps at least duration_min_frames(cfg_d) frames, so the vocoder never sees a length it cannot take:
    an utterance whose table is invalid, or whose total would fall below that, keeps its own timing (flags 1, 2).

    Returns a namedtuple: y_wav_pred [B, max_samples], mel_pred / stft_pred / phn_pred [B, max_frames, C] (warped; zero
    beyond an utterance's extent), the DEVICE tensors n_frames, n_samples (= hop * (n_frames - 1), at out_sr when
    resampled) and flags [B], seg = (labels, start, end, n_seg) the segment table in output frames, map (the
    duration_map_batch result), the host bounds max_frames and max_samples, and src_frames (convert_batch's host
    n_frames).  Nothing is copied back and the host waits for nothing."""
    import audio_lib
    what = 'convert_duration_batch'
    note = " ('numpy' needs host lengths)"
    momentum = _check_momentum(momentum)
    seed = audio_lib.check_seed(seed)
    _need_cfg(cfg_d, what)
    _check_phase(phase, what, None, ('device', 'spsi'), 'max_frames', note)
    if mode not in _WARP_MODES:
        raise ValueError(" - ERROR, {}: mode must be 'linear' or 'nearest', got {!r}".format(what, mode))
    req = _duration_request(what, rate, ratio, gap_ratio, segments, decode, out_len)
    h = _convert_host(what, decoder, wav, lens, cfg_d, t_s, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr,
                      res_type, denoise, dereverb)
    plan, B, hop, Fout = h.plan, h.B, h.hop, h.plan.Fout
    req = _duration_bound(what, req, plan.n_out.astype(np.int64), Fout, duration_min_frames(cfg_d), max_frames,
                          'the vocoder needs {}')
    Fw = req.Fw
    _check_phase(phase, what, (B, Fw, h.n_bins), ('device', 'spsi'), 'max_frames', note)
    req = _duration_decoder(what, req, decoder, encoder, B, Fout)
    _need_gpu(what)

    up = _convert_upload(h, wav, [])
    d_nout = up.d_nout
    phase = _phase_upload(phase)
    _, _, y_mel, y_stft, y_phn = _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type)
    mel_s, phn_s, stft_s, _ = _stitch(y_mel, y_phn, y_stft, up.d_utt, Fout)
    m, seg = _duration_map(what, req, d_nout, phn_s, Fout)        # the segment table in stitched frames, the map

    # ---- the warp, the vocoder
    wm = _WARP_MODES[mode]
    mel_pred = _warp_launch(mel_s, m.pos, m.n_out, d_nout, wm)
    phn_pred = _warp_launch(phn_s, m.pos, m.n_out, d_nout, wm)
    amp_pred = None
    if float(realse) == 1.0:
        stft_pred, amp_pred = _warp_launch(stft_s, m.pos, m.n_out, d_nout, wm, cfg_d['P_dB_norm_factor'])
    else:
        stft_pred = _warp_launch(stft_s, m.pos, m.n_out, d_nout, wm)
    _, y_wav_pred = _vocoder_tail(cfg_d, m.n_out, up.d_ids, n_iter, momentum, realse, seed, phase, phase, None, stft_pred, amp_pred)
    y_wav_pred, n_samples, max_samples = _resample_output_device(y_wav_pred, (hop * (m.n_out - 1)).clamp_min(0), hop * (Fw - 1),
                                                                 h.res_out, cfg_d, out_sr, res_type)
    return _DUR_NT(y_wav_pred, n_samples, mel_pred, stft_pred, phn_pred, m.n_out, m.flags, seg, m, Fw, max_samples,
                   [int(v) for v in plan.n_out])


# --------------------------------------------------------------------------- pitch (csrc/vc_pitch.hip)
PSOLA_MAX_LEN = 1 << 24     # vc_psola_plan, vc_psola_ola_f32: samples per utterance
PSOLA_MAX_FRAMES = 1 << 20
PSOLA_MAX_HOP = 65536
PSOLA_RATIO_MIN, PSOLA_RATIO_MAX = 0.5, 2.0
PSOLA_WIN_N = 2048
_PLAN_PITCH_NT = namedtuple('psola_plan', 'n_a n_s a s src h max_len')
_SHIFT_NT = namedtuple('pitch_shift', 'y plan period_q ratio_q')
_F0_STATS_NT = namedtuple('f0_stats', 'count mean std')
_PITCH_NT = namedtuple('convert_pitch', _BATCH_NT._fields + ('f0_pred', 'f0_target', 'plan'))
_psola_windows = {}


def psola_window(device=None):
    """The one window table of the overlap-add (include/vc_hip.h, "Pitch"): W[i] = float32(0.5 + 0.5 cos(pi i / 2048)),
    i = 0 .. 2048, made in float64, W[2048] = 0.  A numpy array without ``device``; with one, the device's cached copy."""
    w = (0.5 + 0.5 * np.cos(np.pi * np.arange(PSOLA_WIN_N + 1, dtype=np.float64) / PSOLA_WIN_N)).astype(np.float32)
    w[PSOLA_WIN_N] = 0.0
    if device is None:
        return w
    import torch
    key = str(torch.device(device))
    if key not in _psola_windows:
        _psola_windows[key] = torch.from_numpy(w).pin_memory().to(device, non_blocking=True)
    return _psola_windows[key]


def _check_pitch_ratio(r, what):
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not PSOLA_RATIO_MIN <= float(r) <= PSOLA_RATIO_MAX:
        raise ValueError(' - ERROR, {} must be a number in [{}, {}], got {!r}'.format(what, PSOLA_RATIO_MIN, PSOLA_RATIO_MAX, r))
    return float(r)


def pitch_tables(f0_cur, sr, ratio=None, target_f0=None, unvoiced_period=None, hop_length=80):
    """The two Q16 tables of vc_psola_plan from an F0 track: (period_q, ratio_q), int32 in the shape of f0_cur, on its
    device (a numpy array: on the host), computed in float64 torch and rounded once (ties to even).

    f0_cur [B, F] in Hz, 0 = unvoiced (as f0_track_batch returns it).  period_q = round(sr * 65536 / f0) where f0 > 0, else
    unvoiced_period << 16 (default: hop_length samples -- unvoiced stretches are copied grain by grain at the frame rate).
    Exactly one of ratio -- a number in [0.5, 2] or a per-frame array / tensor in the shape of f0_cur -- and target_f0 (the
    contour to reach: ratio_q = round(65536 * target_f0 / f0_cur) where both are voiced, else 65536).  The launch clamps
    what it reads (periods to [16, 1024] samples, ratios to [0.5, 2]); a per-frame ratio on the host is checked here."""
    import torch
    what = 'pitch_tables'
    if (ratio is None) == (target_f0 is None):
        raise ValueError(' - ERROR, {}: pass exactly one of ratio and target_f0'.format(what))
    if isinstance(sr, bool) or not isinstance(sr, (int, float, np.integer, np.floating)) or not 0 < float(sr) <= 2 ** 24:
        raise ValueError(' - ERROR, {}: sr must be a positive number, got {!r}'.format(what, sr))
    if unvoiced_period is None:
        unvoiced_period = hop_length
    if isinstance(unvoiced_period, bool) or not isinstance(unvoiced_period, (int, np.integer)) or not 1 <= unvoiced_period <= 32767:
        raise ValueError(' - ERROR, {}: unvoiced_period must be an integer in [1, 32767], got {!r}'.format(what, unvoiced_period))
    if getattr(f0_cur, 'ndim', 0) != 2 or min(f0_cur.shape) < 1:
        raise ValueError(' - ERROR, {}: f0_cur must be [B, F]'.format(what))
    f0 = torch.as_tensor(f0_cur).to(torch.float64)
    voiced = f0 > 0
    one = torch.ones_like(f0)
    per = torch.where(voiced, torch.round(float(sr) * 65536.0 / torch.where(voiced, f0, one)), one * float(int(unvoiced_period) << 16))
    if target_f0 is not None:
        if tuple(getattr(target_f0, 'shape', ())) != tuple(f0.shape):
            raise ValueError(' - ERROR, {}: target_f0 must have the shape of f0_cur, {}'.format(what, list(f0.shape)))
        tgt = torch.as_tensor(target_f0).to(device=f0.device, dtype=torch.float64)
        both = voiced & (tgt > 0)
        rq = torch.where(both, torch.round(65536.0 * torch.where(both, tgt, one) / torch.where(both, f0, one)), one * 65536.0)
    elif getattr(ratio, 'ndim', 0) == 0:
        rq = one * float(np.rint(65536.0 * _check_pitch_ratio(ratio if not hasattr(ratio, 'item') else ratio.item(), what + ': ratio')))
    else:
        if tuple(ratio.shape) != tuple(f0.shape):
            raise ValueError(' - ERROR, {}: a per-frame ratio must have the shape of f0_cur, {}'.format(what, list(f0.shape)))
        if not torch.is_tensor(ratio):
            r = np.asarray(ratio, dtype=np.float64)
            if not np.isfinite(r).all() or r.min() < PSOLA_RATIO_MIN or r.max() > PSOLA_RATIO_MAX:
                raise ValueError(' - ERROR, {}: ratio must be finite and lie in [{}, {}]'.format(what, PSOLA_RATIO_MIN, PSOLA_RATIO_MAX))
        rq = torch.round(65536.0 * torch.as_tensor(ratio).to(device=f0.device, dtype=torch.float64))
    to_i32 = lambda t: torch.nan_to_num(t, nan=0.0).clamp(0.0, 2.0 ** 31 - 1).to(torch.int32).contiguous()
    return to_i32(per), to_i32(rq)


def _psola_plan_launch(d_per, d_rat, d_lens, Lmax, hop):
    """vc_psola_plan on validated device tensors: no host check, copy or wait in here."""
    import torch
    import _vc
    lib = _vc.lib()
    B, F = d_per.shape
    M = lib.vc_psola_max_marks(Lmax)
    if M == 0:
        raise _vc.VCError('vc_psola_max_marks refused {} samples'.format(Lmax))
    n = torch.empty((2, B), dtype=torch.int32, device=d_per.device)
    tab = torch.empty((4, B, M), dtype=torch.int32, device=d_per.device)
    _vc.check(lib.vc_psola_plan(_vc.ptr(d_per), _vc.ptr(d_rat), _vc.ptr(d_lens), B, Lmax, F, hop, _vc.ptr(n[0]), _vc.ptr(n[1]),
                                _vc.ptr(tab[0]), _vc.ptr(tab[1]), _vc.ptr(tab[2]), _vc.ptr(tab[3]), _vc.current_stream()))
    return _PLAN_PITCH_NT(n[0], n[1], tab[0], tab[1], tab[2], tab[3], Lmax)


def _psola_ola_launch(wav, d_lens, plan, w_floor):
    """vc_psola_ola_f32 on validated device tensors (wav [B, plan.max_len] contiguous float32)."""
    import torch
    import _vc
    B, Lmax = wav.shape
    y = torch.empty_like(wav)
    _vc.check(_vc.lib().vc_psola_ola_f32(_vc.ptr(wav), _vc.ptr(d_lens), _vc.ptr(plan.n_s), _vc.ptr(plan.s), _vc.ptr(plan.src),
                                         _vc.ptr(plan.h), _vc.ptr(psola_window(wav.device)), B, Lmax, w_floor, _vc.ptr(y),
                                         _vc.current_stream()))
    return y


def _check_pitch_sizes(B, Lmax, F, hop, what):
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or not 1 <= hop <= PSOLA_MAX_HOP:
        raise ValueError(' - ERROR, {}: hop_length must be an integer in [1, {}], got {!r}'.format(what, PSOLA_MAX_HOP, hop))
    if isinstance(Lmax, bool) or not isinstance(Lmax, (int, np.integer)) or not 1 <= Lmax <= PSOLA_MAX_LEN:
        raise ValueError(' - ERROR, {}: at most {} samples per utterance, at least 1 (got {!r})'.format(what, PSOLA_MAX_LEN, Lmax))
    if not 1 <= B <= 65535 or not 1 <= F <= PSOLA_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: 1 to 65535 utterances of 1 to {} frames (got {} of {})'.format(what, PSOLA_MAX_FRAMES, B, F))


def _check_pitch_lens(lens, B, Lmax, what):
    import torch
    if torch.is_tensor(lens) and lens.is_cuda:
        return
    h = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > Lmax:
        raise ValueError(' - ERROR, {}: lens must be {} integers in [0, {}]'.format(what, B, Lmax))


def _check_w_floor(w_floor, what):
    if isinstance(w_floor, bool) or not isinstance(w_floor, (int, float, np.integer, np.floating)) or not 0.0 < float(w_floor) <= 2.0:
        raise ValueError(' - ERROR, {}: w_floor must be a number in (0, 2], got {!r}'.format(what, w_floor))
    return float(w_floor)


def _check_pitch_table(t, B, what):
    import torch
    if getattr(t, 'ndim', 0) != 2 or t.shape[0] != B or t.shape[1] < 1:
        raise ValueError(' - ERROR, {} must be [B, F]'.format(what))
    return _i32_device(t, tuple(t.shape), what)


def psola_plan_batch(period_q, ratio_q, lens, hop_length, max_len=None):
    """The grain plan of B utterances (vc_psola_plan; the definition is in include/vc_hip.h, "Pitch", the numpy restatement
    in tests/pitch_ref.py).  period_q, ratio_q [B, F] int32 as pitch_tables returns them; lens: the sample counts, host
    integers or an int32 [B] device tensor; max_len: the bound Lmax of the lengths (default: the largest of host lens,
    required with lens on the device).  Returns a namedtuple of device tensors: n_a, n_s [B] (the numbers K, J of analysis
    and synthesis marks), a, s, src, h [B, max_len // 16 + 1] int32 (-1 beyond), and the host integer max_len.  Nothing is
    copied back and the host waits for nothing."""
    import torch
    what = 'psola_plan_batch'
    if getattr(period_q, 'ndim', 0) != 2 or tuple(getattr(ratio_q, 'shape', ())) != tuple(period_q.shape):
        raise ValueError(' - ERROR, {}: period_q and ratio_q must be [B, F], the same shape'.format(what))
    B, F = int(period_q.shape[0]), int(period_q.shape[1])
    if max_len is None:
        if torch.is_tensor(lens) and lens.is_cuda:
            raise ValueError(' - ERROR, {}: max_len is required with lens on the device'.format(what))
        max_len = max(int(np.max(np.asarray(lens))), 1) if np.size(lens) else 1
    _check_pitch_sizes(B, max_len, F, hop_length, what)
    _check_pitch_lens(lens, B, max_len, what)
    _need_gpu(what)
    return _psola_plan_launch(_check_pitch_table(period_q, B, what + ': period_q'), _check_pitch_table(ratio_q, B, what + ': ratio_q'),
                              _i32_device(lens, (B,), what + ': lens'), int(max_len), int(hop_length))


def pitch_shift_batch(wav, lens, f0, sr, hop_length, ratio=None, target_f0=None, w_floor=0.5, unvoiced_period=None):
    """Changes the fundamental of B waveforms and keeps their lengths: pitch_tables, vc_psola_plan, vc_psola_ola_f32.

    wav [B, Lmax] float32 (cuda tensor or numpy array); lens: sample counts, host integers, an int32 [B] device tensor (as
    convert_duration_batch returns n_samples) or None (all Lmax); f0 [B, F] in Hz, 0 = unvoiced, the track of ``wav`` at
    ``hop_length`` (f0_track_batch's f0; F need not be 1 + Lmax // hop_length: the last frame extends to the end).  One of
    ratio (a number in [0.5, 2] or per frame) and target_f0 [B, F].  w_floor: the least window sum an output sample is
    divided by (a sample that fewer grains reach is damped, not amplified).
    Returns a namedtuple: y [B, Lmax] float32 on the device (zero from an utterance's length on), the plan
    (psola_plan_batch's result) and the two tables.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'pitch_shift_batch'
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    if torch.is_tensor(wav) and wav.dtype != torch.float32:
        raise ValueError(' - ERROR, {}: wav must be float32, got {}'.format(what, wav.dtype))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    if getattr(f0, 'ndim', 0) != 2 or f0.shape[0] != B or f0.shape[1] < 1:
        raise ValueError(' - ERROR, {}: f0 must be [B, F] with B = {}'.format(what, B))
    _check_pitch_sizes(B, Lmax, int(f0.shape[1]), hop_length, what)
    w_floor = _check_w_floor(w_floor, what)
    if lens is None:
        lens = np.full((B,), Lmax, dtype=np.int64)
    _check_pitch_lens(lens, B, Lmax, what)
    _need_gpu(what)
    if not torch.is_tensor(f0):
        f0 = torch.from_numpy(np.ascontiguousarray(f0))
    if torch.is_tensor(ratio) or torch.is_tensor(target_f0):
        ratio, target_f0 = (t.to('cuda', non_blocking=True) if torch.is_tensor(t) else t for t in (ratio, target_f0))
    per, rat = pitch_tables(f0.to('cuda', non_blocking=True), sr, ratio=ratio, target_f0=target_f0, unvoiced_period=unvoiced_period,
                            hop_length=int(hop_length))
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    d_lens = _i32_device(lens, (B,), what + ': lens')
    plan = _psola_plan_launch(per, rat, d_lens, Lmax, int(hop_length))
    return _SHIFT_NT(_psola_ola_launch(wav, d_lens, plan, w_floor), plan, per, rat)


def f0_stats_batch(f0, n_frames=None):
    """Count, mean and standard deviation (population) of log F0 over the voiced frames of a batch of tracks, pooled:
    f0 [B, F] in Hz, 0 = unvoiced; n_frames [B] (host integers or a tensor; None = all F): frames from it on are left out.
    A namedtuple (count int64, mean, std float64) of 0-d tensors on f0's device; without a voiced frame mean = std = 0.
    Plain torch: no kernel of this library, nothing copied back."""
    import torch
    if getattr(f0, 'ndim', 0) != 2:
        raise ValueError(' - ERROR, f0_stats_batch: f0 must be [B, F]')
    f0 = torch.as_tensor(f0)
    B, F = f0.shape
    keep = f0 > 0
    if n_frames is not None:
        n = torch.as_tensor(n_frames).to(f0.device).reshape(-1)
        if n.shape[0] != B:
            raise ValueError(' - ERROR, f0_stats_batch: n_frames must hold {} counts'.format(B))
        keep = keep & (torch.arange(F, device=f0.device)[None, :] < n[:, None])
    lf = torch.where(keep, torch.log(torch.where(keep, f0, torch.ones_like(f0)).to(torch.float64)), torch.zeros((), dtype=torch.float64, device=f0.device))
    count = keep.sum()
    den = count.clamp_min(1).to(torch.float64)
    mean = lf.sum() / den
    var = (torch.where(keep, lf - mean, torch.zeros_like(lf)) ** 2).sum() / den
    return _F0_STATS_NT(count, mean, torch.sqrt(var))


def f0_transform(f0, stats_src, stats_tgt):
    """The log-Gaussian mapping of an F0 contour from one speaker's statistics to another's:
    exp((log f0 - mean_src) * std_tgt / std_src + mean_tgt) where f0 > 0; unvoiced frames stay 0.  Where std_src is 0 the
    contour is moved by the means alone.  stats_*: (count, mean, std) as f0_stats_batch returns them (tensors or numbers).
    float32 on f0's device; no synchronisation."""
    import torch
    if len(stats_src) != 3 or len(stats_tgt) != 3:
        raise ValueError(' - ERROR, f0_transform: stats must be (count, mean, std) as f0_stats_batch returns them')
    f0 = torch.as_tensor(f0)
    as64 = lambda v: torch.as_tensor(v).to(device=f0.device, dtype=torch.float64)
    ms, ss, mt, st = as64(stats_src[1]), as64(stats_src[2]), as64(stats_tgt[1]), as64(stats_tgt[2])
    voiced = f0 > 0
    lf = torch.log(torch.where(voiced, f0, torch.ones_like(f0)).to(torch.float64))
    slope = torch.where(ss > 0, st / torch.where(ss > 0, ss, torch.ones_like(ss)), torch.ones_like(ss))
    out = torch.exp((lf - ms) * slope + mt)
    return torch.where(voiced, out, torch.zeros_like(out)).to(torch.float32)


def _tracker_keys(f0_args, what):
    """f0_args (a dict of f0_track_batch's tracker arguments, or None): the keys checked, the defaults filled in."""
    kw = dict(frame_length=512, fmin=60.0, fmax=400.0, threshold=0.15, jump_cost=0.5, switch_cost=0.1, n_cand=8, ceiling=1.0)
    extra = set(f0_args or {}) - set(kw)
    if extra:
        raise ValueError(' - ERROR, {}: f0_args takes {}, got {}'.format(what, sorted(kw), sorted(extra)))
    kw.update(f0_args or {})
    return kw


def _tracker_args(kw, sr, hop, what):
    """The values of _tracker_keys' dict checked on the host: (f0a, n_cand, ceiling, costs) as evaluation._f0_track_launch
    takes them."""
    import evaluation
    f0a = evaluation._f0_args(sr, hop, kw['frame_length'], kw['fmin'], kw['fmax'], kw['threshold'], what)
    n_cand, ceiling = evaluation._track_args(kw['n_cand'], kw['ceiling'], what)
    return f0a, n_cand, ceiling, evaluation._viterbi_costs(f0a[5], kw['jump_cost'], kw['switch_cost'], what)


def _parse_pitch(pitch, stats_src, stats_tgt, what, none_ok, stats_kinds, forms, stats_with):
    """pitch= of convert_pitch_batch, convert_hnm_batch and convert_diff_batch: (kind, value) with kind None, 'source', 'ratio'
    (value: the checked float) or 'contour' (its shape is checked once the plan is known: _check_contour).  none_ok: whether
    pitch=None is a request; stats_kinds: the kinds that stats_src / stats_tgt may come with.  forms, stats_with: the
    caller's wording of the choices and of that rule, for its messages."""
    source = isinstance(pitch, str)
    if (pitch is None and not none_ok) or (source and pitch != 'source'):
        raise ValueError(' - ERROR, {}: pitch must be {}, got {!r}'.format(what, forms, pitch))
    kind = None if pitch is None else 'source' if source else 'ratio' if getattr(pitch, 'ndim', 0) == 0 else 'contour'
    if (stats_src is None) != (stats_tgt is None) or (stats_src is not None and kind not in stats_kinds):
        raise ValueError(' - ERROR, {}: stats_src and stats_tgt go together and with {}'.format(what, stats_with))
    if kind == 'ratio':
        pitch = _check_pitch_ratio(pitch, what + ': pitch')
    return kind, pitch


def _check_contour(kind, pitch, B, Fout, what, per='output frame'):
    if kind == 'contour' and tuple(getattr(pitch, 'shape', ())) != (B, Fout):
        raise ValueError(' - ERROR, {}: a pitch contour must be [{}, {}] (Hz per {})'.format(what, B, Fout, per))


def _contour_upload(kind, pitch):
    """A contour given on the host goes up pinned; every other kind of pitch= passes through."""
    import torch
    if kind != 'contour':
        return pitch
    if not torch.is_tensor(pitch):
        pitch = torch.from_numpy(np.ascontiguousarray(pitch, dtype=np.float32)).pin_memory()
    return pitch.to(device='cuda', non_blocking=True)


def _source_contour(up, d_fout, d_fsrc, Fout, tracker, stats_src, stats_tgt):
    """pitch='source' on the device: the input's contour (up.wav at the model's rate, tracked by f0_track_batch's launches),
    aligned to the output frames by the plan's n_s (output frame u is input frame n_s + u; up.d_true[:, 1]) and mapped by
    f0_transform when the speakers' statistics are given.  [B, Fout] float32, 0 beyond an utterance's frames."""
    import torch
    import evaluation
    f0_in = evaluation._f0_track_launch(up.wav, up.d_lens, d_fsrc, *tracker)[0]
    u = torch.arange(Fout, device=f0_in.device)[None, :]
    idx = up.d_true[:, 1:2].long() + u
    ok = (u < d_fout[:, None]) & (idx < d_fsrc[:, None])
    f0_target = torch.where(ok, torch.gather(f0_in, 1, idx.clamp(0, f0_in.shape[1] - 1)), torch.zeros((), device=f0_in.device))
    if stats_src is not None:
        f0_target = f0_transform(f0_target, stats_src, stats_tgt)
    return f0_target


def convert_pitch_batch(decoder, wav, lens=None, cfg_d=None, pitch=None, stats_src=None, stats_tgt=None, w_floor=0.5, f0_args=None,
                        t_s=0, t_e=60, n_iter=200, realse=1.0, two_pass=True, momentum=0.0, phase='device', seed=0, utt_ids=None,
                        window_batch=64, encoder=None, wav_sr=None, out_sr=None, res_type='kaiser_best', denoise=None,
                        dereverb=None):
    """``convert_batch`` with the melody set as well: after the vocoder the converted waveform's F0
    is tracked (f0_track_batch's launches, at the model's rate and hop), and pitch_shift_batch's launches move it to the
    target before the output is resampled.

    pitch:
      a number r         every voiced frame's fundamental times r (0.5 <= r <= 2);
      [B, Fout] floats   the contour to reach, in Hz per output frame, 0 = leave the frame as it is;
      'source'           the INPUT's own contour: tracked on ``wav`` at the model's rate, mapped by
                         f0_transform(., stats_src, stats_tgt) when both are given (f0_stats_batch of the two speakers),
                         and aligned to the output frames by the plan's n_s (output frame u is input frame n_s + u).
    f0_args: a dict of f0_track_batch's tracker arguments (frame_length, fmin, fmax, threshold, jump_cost, switch_cost,
    n_cand, ceiling).  The other arguments are convert_batch's; phase='numpy' and giffin_lim_input are not offered here.
    denoise: as convert_batch's -- the input is denoised once, at the model's rate, before the model, a tracker or a
    filter reads it, and mel_true / stft_true are those of the denoised input.
    Returns convert_batch's fields (y_wav_true None) plus f0_pred [B, Fout] (the track of the unshifted conversion),
    f0_target [B, Fout] (None for a number) and the grain plan.  Every check and table is made on the host before the first
    launch; after the uploads nothing is copied to the host and the host waits for nothing."""
    import torch
    import audio_lib
    import evaluation
    what = 'convert_pitch_batch'
    momentum = _check_momentum(momentum)
    seed = audio_lib.check_seed(seed)
    _need_cfg(cfg_d, what)
    _check_phase(phase, what)
    if pitch is None:
        raise ValueError(" - ERROR, {}: pitch is required: a ratio, a [B, Fout] contour or 'source'".format(what))
    kind, pitch = _parse_pitch(pitch, stats_src, stats_tgt, what, False, ('source',), "a ratio, a [B, Fout] contour or 'source'",
                               "pitch='source'")
    w_floor = _check_w_floor(w_floor, what)
    tracker = _tracker_args(_tracker_keys(f0_args, what), cfg_d['sample_rate'], int(cfg_d['hop_length']), what)
    h = _convert_host(what, decoder, wav, lens, cfg_d, t_s, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr,
                      res_type, denoise, dereverb)
    plan, B, hop, Fout, sr = h.plan, h.B, h.hop, h.plan.Fout, cfg_d['sample_rate']
    Lout = hop * (Fout - 1)
    _check_pitch_sizes(B, Lout, Fout, hop, what)
    if max(Lout, int(h.h_lens.max())) > evaluation.F0_MAX_SAMPLES:
        raise ValueError(' - ERROR, {}: the tracker takes at most {} samples per utterance'.format(what, evaluation.F0_MAX_SAMPLES))
    _check_phase(phase, what, (B, Fout, h.n_bins))
    _check_contour(kind, pitch, B, Fout, what)
    _need_gpu(what)

    up = _convert_upload(h, wav, [h.h_nsamp, plan.n_out, plan.n_src])
    d_nsamp, d_fout, d_fsrc = up.d_extra[-3:]
    phase = _phase_upload(phase)
    pitch = _contour_upload(kind, pitch)
    psola_window('cuda')
    h, up = _resample_input(h, up, cfg_d, wav_sr, res_type)       # here: the source's track needs the model's rate too
    h, up = _denoise_input(h, up, cfg_d, h.denoise)

    # ---- convert_batch's model pass, stitch and vocoder
    mel_true, stft_true, y_mel, y_stft, y_phn = _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type)
    mel_pred, phn_pred, stft_pred, amp_pred = _stitch(y_mel, y_phn, y_stft, up.d_utt, Fout,
                                                      cfg_d['P_dB_norm_factor'] if float(realse) == 1.0 else None)
    _, y0 = _vocoder_tail(cfg_d, up.d_nout, up.d_ids, n_iter, momentum, realse, seed, phase, phase, None, stft_pred, amp_pred)

    # ---- the conversion's own track, the target, the shift
    f0_pred = evaluation._f0_track_launch(y0, d_nsamp, d_fout, *tracker)[0]
    f0_target = None
    if kind == 'source':
        f0_target = _source_contour(up, d_fout, d_fsrc, Fout, tracker, stats_src, stats_tgt)
    elif kind == 'contour':
        f0_target = pitch.to(torch.float32)
    per, rat = pitch_tables(f0_pred, sr, ratio=pitch if kind == 'ratio' else None, target_f0=f0_target, hop_length=hop)
    pp = _psola_plan_launch(per, rat, d_nsamp, Lout, hop)
    y_wav_pred, n_samples = _resample_output(_psola_ola_launch(y0, d_nsamp, pp, w_floor), h.h_nsamp, d_nsamp, h.res_out, cfg_d,
                                             out_sr, res_type)
    return _PITCH_NT(None, y_wav_pred, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred, [int(v) for v in plan.n_out],
                     f0_pred, f0_target, pp)


_HNM_NT = namedtuple('convert_hnm', _BATCH_NT._fields + ('f0_target', 'env_log', 'plan'))


def convert_hnm_batch(decoder, wav, lens=None, cfg_d=None, pitch='source', stats_src=None, stats_tgt=None, f0_args=None, order=24,
                      iters=16, voiced_cutoff_hz=4000.0, noise_level=1.0, realse=1.0, floor=1e-5, f0_lo=40.0, f0_hi=None, t_s=0,
                      t_e=60, two_pass=True, seed=0, utt_ids=None, window_batch=64, encoder=None, wav_sr=None, out_sr=None,
                      res_type='kaiser_best', denoise=None,
                      dereverb=None):
    """``convert_batch`` with the harmonic-plus-noise vocoder in Griffin-Lim's place: the decoder's
    spectrum gives the envelope, an F0 contour the excitation, and audio_lib.hnm_synth_batch's launches write the waveform
    in one pass -- no phase iteration, and the pitch is the one asked for.

    pitch:
      'source'           the INPUT's own contour, tracked on ``wav`` at the model's rate, aligned to the output frames by the
                         plan's n_s and mapped by f0_transform(., stats_src, stats_tgt) when both are given;
      a number r         that contour times r (0.5 <= r <= 2);
      [B, Fout] floats   the contour itself, Hz per output frame, 0 = unvoiced.
    f0_args: the tracker's arguments as in convert_pitch_batch; order, iters, floor: envelope_batch's; voiced_cutoff_hz,
    noise_level, seed, utt_ids, f0_lo, f0_hi: hnm_synth_batch's.  The magnitude is made as convert_batch makes it (fused in
    the stitch at realse == 1, else vc_power_to_amp); after the synthesiser come convert_batch's de-emphasis and level
    (the spectra are those of the pre-emphasised signal) and the resampling to out_sr.
    denoise: as convert_batch's -- the input is denoised once, at the model's rate, before the model, a tracker or a
    filter reads it, and mel_true / stft_true are those of the denoised input.
    Returns convert_batch's fields (y_wav_true None) plus f0_target [B, Fout], env_log [B, Fout, bins] and the phase plan.
    Every check and table is made on the host before the first launch; after the uploads nothing is copied to the host and
    the host waits for nothing."""
    import torch
    import audio_lib
    what = 'convert_hnm_batch'
    seed = audio_lib.check_seed(seed)
    _need_cfg(cfg_d, what)
    kind, pitch = _parse_pitch(pitch, stats_src, stats_tgt, what, False, ('source', 'ratio'),
                               "'source', a ratio or a [B, Fout] contour", "the source's contour")
    sr, hop = int(cfg_d['sample_rate']), int(cfg_d['hop_length'])
    tracker = None if kind == 'contour' else _tracker_args(_tracker_keys(f0_args, what), sr, hop, what)
    h = _convert_host(what, decoder, wav, lens, cfg_d, t_s, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr,
                      res_type, denoise, dereverb)
    plan, B, Fout, n_bins = h.plan, h.B, h.plan.Fout, h.n_bins
    n_fft, order, iters, floor = audio_lib._check_envelope_args(what, (B, Fout, n_bins), h.n_fft, order, iters, floor)
    _, _, f0_lo, f0_hi = audio_lib._check_plan_args(what, (B, Fout), sr, hop, f0_lo, f0_hi)
    cutoff = audio_lib.hnm_cutoff(voiced_cutoff_hz, sr, n_fft, f0_lo)
    noise_level = audio_lib._hnm_float(noise_level, what, 'noise_level', lo=0.0)
    _check_contour(kind, pitch, B, Fout, what)
    if kind != 'contour':
        import evaluation
        if int(h.h_lens.max()) > evaluation.F0_MAX_SAMPLES:
            raise ValueError(' - ERROR, {}: the tracker takes at most {} samples per utterance'.format(what, evaluation.F0_MAX_SAMPLES))
    _need_gpu(what)

    up = _convert_upload(h, wav, [h.h_nsamp, plan.n_out, plan.n_src])
    d_nsamp, d_fout, d_fsrc = up.d_extra[-3:]
    pitch = _contour_upload(kind, pitch)
    h, up = _resample_input(h, up, cfg_d, wav_sr, res_type)       # here: the source's track needs the model's rate too
    h, up = _denoise_input(h, up, cfg_d, h.denoise)

    # ---- convert_batch's model pass and stitch, the magnitude as convert_batch makes it
    mel_true, stft_true, y_mel, y_stft, y_phn = _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type)
    mel_pred, phn_pred, stft_pred, amp_pred = _stitch(y_mel, y_phn, y_stft, up.d_utt, Fout,
                                                      cfg_d['P_dB_norm_factor'] if float(realse) == 1.0 else None)
    if amp_pred is None:
        amp_pred = _power_to_amp(stft_pred, up.d_nout, cfg_d, realse)

    # ---- the contour, the synthesiser, de-emphasis and level
    if kind == 'contour':
        f0_target = pitch.to(torch.float32).contiguous()
    else:
        f0_target = _source_contour(up, d_fout, d_fsrc, Fout, tracker, stats_src, stats_tgt)
        if kind == 'ratio':
            f0_target = f0_target * float(pitch)
    vplan = audio_lib._get_voc_plan(cfg_d['win_length'], hop, n_fft)
    syn = audio_lib._hnm_chain(vplan, amp_pred, f0_target, up.d_nout, d_nsamp, sr, order, iters, floor, f0_lo, f0_hi, cutoff,
                               noise_level, seed, up.d_ids, noise_level > 0.0)
    y_wav_pred = _deemphasis_level(vplan, syn.y, up.d_nout, Fout, cfg_d, cfg_d['pre_emphasis'])
    y_wav_pred, n_samples = _resample_output(y_wav_pred, h.h_nsamp, d_nsamp, h.res_out, cfg_d, out_sr, res_type)
    return _HNM_NT(None, y_wav_pred, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred, [int(v) for v in plan.n_out],
                   f0_target, syn.env_log, syn.plan)


# --------------------------------------------------------------------------- differential spectrum (csrc/vc_vocoder.hip)
DIFF_MAX_HALF_WIDTH = 32    # vc_spectral_diff_gain_f32: at most 65 taps
_DIFF_NT = namedtuple('convert_diff', 'y_wav_pred n_samples mel_true mel_pred stft_true stft_pred phn_pred gain n_frames f0_src')


def diff_smoothing_taps(half_width=8):
    """The smoothing taps of the differential gain along frequency: a Hann shape over 2 * half_width + 1 bins,
    0.5 + 0.5 cos(pi j / (half_width + 1)) for j = -half_width .. half_width (no zero end taps), computed in float64,
    normalised to sum 1 and rounded to float32; half_width = 0 gives the single tap 1.  Host only."""
    if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or not 0 <= half_width <= DIFF_MAX_HALF_WIDTH:
        raise ValueError(' - ERROR, diff_smoothing_taps: half_width must be an integer in [0, {}], got {!r}'.format(DIFF_MAX_HALF_WIDTH, half_width))
    h = int(half_width)
    c = 0.5 + 0.5 * np.cos(np.pi * np.arange(-h, h + 1, dtype=np.float64) / (h + 1))
    c = 0.5 * (c + c[::-1])                                          # symmetric to the last bit
    return (c / c.sum()).astype(np.float32)


def _check_diff_args(alpha, max_boost_db, max_cut_db, what):
    out = []
    for v, name, hi in ((alpha, 'alpha', 1.0), (max_boost_db, 'max_boost_db', None), (max_cut_db, 'max_cut_db', None)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= float(np.finfo(np.float32).max) \
                or (hi is not None and float(v) > hi):                  # NaN fails the comparison; finite as a float32
            raise ValueError(' - ERROR, {}: {} must be a finite number {}, got {!r}'.format(
                what, name, 'in [0, 1]' if hi is not None else 'that is not negative', v))
        out.append(float(v))
    return tuple(out)


def _check_diff_taps(half_width, taps, what):
    """float32 [n_taps] on the host: ``taps`` when given (odd, at most 65, finite), else diff_smoothing_taps(half_width)."""
    if taps is None:
        return diff_smoothing_taps(half_width)
    import torch
    t = np.asarray(taps.cpu() if torch.is_tensor(taps) else taps, dtype=np.float32)
    if t.ndim != 1 or t.size % 2 != 1 or t.size > 2 * DIFF_MAX_HALF_WIDTH + 1 or not np.isfinite(t).all():
        raise ValueError(' - ERROR, {}: taps must be an odd number of finite floats, at most {}'.format(what, 2 * DIFF_MAX_HALF_WIDTH + 1))
    return np.ascontiguousarray(t)


def _diff_gain_launch(stft_pred, stft_true, d_nf, norm, alpha, boost, cut, d_taps):
    """vc_spectral_diff_gain_f32 on validated device tensors: no host check, copy or wait in here."""
    import torch
    import _vc
    B, F, nb = stft_pred.shape
    gain = torch.empty_like(stft_pred)
    _vc.check(_vc.lib().vc_spectral_diff_gain_f32(_vc.ptr(stft_pred), _vc.ptr(stft_true), _vc.ptr(d_nf), B, F, nb, norm, alpha, boost,
                                                  cut, _vc.ptr(d_taps), d_taps.shape[0], _vc.ptr(gain), _vc.current_stream()))
    return gain


def diff_gain_batch(stft_pred, stft_true, n_frames, P_dB_norm_factor, alpha=1.0, max_boost_db=20.0, max_cut_db=30.0, half_width=8,
                    taps=None):
    """The gain of the differential filter (vc_spectral_diff_gain_f32; the definition is in include/vc_hip.h,
    "Differential-spectrum conversion", the restatement in tests/diff_ref.py): per frame and bin the difference of the two
    spectra in dB, smoothed along frequency by ``taps`` (default diff_smoothing_taps(half_width)), scaled by alpha, clamped
    to [-max_cut_db, max_boost_db] and turned into an amplitude ratio.

    stft_pred, stft_true [B, F, bins] float32: the front-end's normalised power dB, as convert_batch(vocode=False) returns
    them.  n_frames: host integers, an int32 [B] device tensor or None (all F).  Returns the gain [B, F, bins] float32 on
    the device, 0 in the rows at or beyond n_frames.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'diff_gain_batch'
    alpha, boost, cut = _check_diff_args(alpha, max_boost_db, max_cut_db, what)
    h_taps = _check_diff_taps(half_width, taps, what)
    norm = float(P_dB_norm_factor)
    if not np.isfinite(norm) or norm == 0.0:
        raise ValueError(' - ERROR, {}: P_dB_norm_factor must be finite and not 0'.format(what))
    if getattr(stft_pred, 'ndim', 0) != 3 or tuple(getattr(stft_true, 'shape', ())) != tuple(stft_pred.shape) or min(stft_pred.shape) < 1:
        raise ValueError(' - ERROR, {}: stft_pred and stft_true must be [B, F, bins], the same shape'.format(what))
    B, F, nb = (int(v) for v in stft_pred.shape)
    if B > 65535 or not 2 <= nb <= 2049:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of 2 to 2049 bins'.format(what))
    if n_frames is not None and not (torch.is_tensor(n_frames) and n_frames.is_cuda):
        h = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > F:
            raise ValueError(' - ERROR, {}: n_frames must be {} integers in [0, {}]'.format(what, B, F))
    _need_gpu(what)
    as_dev = lambda t: (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))).to(
        device='cuda', dtype=torch.float32).contiguous()
    d_nf = None if n_frames is None else _i32_device(n_frames, (B,), what + ': n_frames')
    d_taps = torch.from_numpy(h_taps).pin_memory().to('cuda', non_blocking=True)
    return _diff_gain_launch(as_dev(stft_pred), as_dev(stft_true), d_nf, norm, alpha, boost, cut, d_taps)


def diff_frames(plan, hop):
    """(n_use [B], n_samples [B]) int64 on the host from a convert_plan: n_use = min(n_out, n_clip), the frames of an
    utterance that the model converted AND the source covers; n_samples = hop * (n_use - 1)."""
    n_use = np.minimum(plan.n_out, plan.n_clip).astype(np.int64)
    return n_use, int(hop) * (n_use - 1)


def convert_diff_batch(decoder, wav, lens=None, cfg_d=None, alpha=1.0, max_boost_db=20.0, max_cut_db=30.0, half_width=8, pitch=None,
                       stats_src=None, stats_tgt=None, w_floor=0.5, f0_args=None, t_e=60, two_pass=True, utt_ids=None,
                       window_batch=64, encoder=None, wav_sr=None, out_sr=None, res_type='kaiser_best', denoise=None,
                       dereverb=None):
    """``convert_batch`` without a vocoder: the source recording is FILTERED by the difference between
    the converted and the source spectral envelope (diff_gain_batch, audio_lib.stft_filter_batch), so its excitation and
    phase stay natural and the waveform costs one transform pass instead of a Griffin-Lim run.  t_s is fixed at 0: output
    frame u is input frame u, and the output covers n_use = min(n_out, n_clip) frames of convert_plan per utterance -- the
    whole windows the model converted, cut where the source ends.

    alpha, max_boost_db, max_cut_db, half_width: diff_gain_batch's (none of the defaults is tuned by ear).
    pitch: None, or what moves the SOURCE's fundamental before the filter (pitch_shift_batch's launches on a track of the
    source at the model's rate; the overlap-add keeps the envelope, which the filter then converts):
      a number r         every voiced frame's fundamental times r (0.5 <= r <= 2);
      [B, Fout] floats   the contour to reach, in Hz per frame, 0 = leave the frame as it is;
      'source'           the source's own contour mapped by f0_transform(., stats_src, stats_tgt): both are required.
    w_floor, f0_args: as convert_pitch_batch.  The other arguments are convert_batch's.
    dereverb: as convert_batch's; the room of the source recording would otherwise pass straight to the output.
    denoise: as convert_batch's -- here it matters most: the filter passes the SOURCE recording, so with denoise the tracker
    and the filter read the denoised waveform, and mel_true / stft_true (hence the gain) are those of the denoised input.
    Returns a namedtuple: y_wav_pred [B, hop * (Fout - 1)] (the filtered source at the level convert_batch sets,
    15 * mean_abs_amp_norm; zero beyond an utterance's n_samples), n_samples (hop * (n_use - 1) on the host, at out_sr when
    given), mel_true / mel_pred / stft_true / stft_pred / phn_pred as convert_batch(vocode=False) returns them, gain
    [B, Fout, bins], n_frames (n_use on the host) and f0_src (the source's track [B, 1 + Lmax // hop], None without pitch).
    Every check and table is made on the host before the first launch; after the uploads nothing is copied to the host and
    the host waits for nothing."""
    import torch
    import audio_lib
    import evaluation
    what = 'convert_diff_batch'
    _need_cfg(cfg_d, what)
    alpha, boost, cut = _check_diff_args(alpha, max_boost_db, max_cut_db, what)
    h_taps = _check_diff_taps(half_width, None, what)
    if hasattr(pitch, 'item') and getattr(pitch, 'ndim', None) == 0:
        pitch = pitch.item()                                        # a 0-d array or tensor counts as a number here
    kind, pitch = _parse_pitch(pitch, stats_src, stats_tgt, what, True, ('source',),
                               "None, a ratio, a [B, Fout] contour or 'source'", "pitch='source'")
    if kind == 'source' and stats_src is None:
        raise ValueError(" - ERROR, {}: pitch='source' needs stats_src and stats_tgt (the source's own contour unmapped changes nothing)".format(what))
    if kind == 'source' and (len(stats_src) != 3 or len(stats_tgt) != 3):
        raise ValueError(' - ERROR, {}: stats must be (count, mean, std) as f0_stats_batch returns them'.format(what))
    w_floor = _check_w_floor(w_floor, what)
    f0_kw = _tracker_keys(f0_args, what)
    h = _convert_host(what, decoder, wav, lens, cfg_d, 0, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr, res_type,
                      denoise, dereverb)
    plan, B, hop, Fout, sr = h.plan, h.B, h.hop, h.plan.Fout, cfg_d['sample_rate']
    n_use, h_nsamp = diff_frames(plan, hop)
    if int(h_nsamp.min()) <= h.n_fft // 2:
        raise ValueError(' - ERROR, {}: every utterance needs hop_length*(frames-1) > n_fft//2 samples'.format(what))
    Lmax = int(audio_lib.resample_len(int(wav.shape[1]), wav_sr, sr)) if h.res_in else int(wav.shape[1])
    if kind is not None:
        tracker = _tracker_args(f0_kw, sr, hop, what)
        _check_pitch_sizes(B, Lmax, 1 + Lmax // hop, hop, what)
        if Lmax > evaluation.F0_MAX_SAMPLES:
            raise ValueError(' - ERROR, {}: the tracker takes at most {} samples per utterance'.format(what, evaluation.F0_MAX_SAMPLES))
        _check_contour(kind, pitch, B, Fout, what, 'frame')
    _need_gpu(what)

    # ---- uploads: the waveforms if they are on the host, one table, the taps, a contour
    up = _convert_upload(h, wav, [n_use, h_nsamp, plan.n_src])
    d_nuse, d_nsamp, d_fsrc = up.d_extra[-3:]
    d_taps = torch.from_numpy(h_taps).pin_memory().to('cuda', non_blocking=True)
    pitch = _contour_upload(kind, pitch)
    if kind is not None:
        psola_window('cuda')
    h, up = _resample_input(h, up, cfg_d, wav_sr, res_type)       # here: the filter and the tracker need the model's rate too
    h, up = _denoise_input(h, up, cfg_d, h.denoise)

    # ---- convert_batch(vocode=False): front-end, windows, model, the three stitches
    mel_true, stft_true, y_mel, y_stft, y_phn = _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type)
    mel_pred, phn_pred, stft_pred, _ = _stitch(y_mel, y_phn, y_stft, up.d_utt, Fout)

    # ---- the source's fundamental, moved before the filter
    x, f0_src = up.wav, None
    if kind is not None:
        f0_src = evaluation._f0_track_launch(x, up.d_lens, d_fsrc, *tracker)[0]
        target = None
        if kind == 'source':
            target = f0_transform(f0_src, stats_src, stats_tgt)
        elif kind == 'contour':
            n = min(Fout, f0_src.shape[1])                          # t_s == 0: frame u of the contour is frame u of the source
            target = torch.zeros_like(f0_src)
            target[:, :n] = pitch[:, :n].to(torch.float32)
        per, rat = pitch_tables(f0_src, sr, ratio=pitch if kind == 'ratio' else None, target_f0=target, hop_length=hop)
        x = _psola_ola_launch(x, up.d_lens, _psola_plan_launch(per, rat, up.d_lens, x.shape[1], hop), w_floor)

    # ---- gain, filter, level
    gain = _diff_gain_launch(stft_pred, stft_true, d_nuse, float(cfg_d['P_dB_norm_factor']), alpha, boost, cut, d_taps)
    vplan = audio_lib._get_voc_plan(cfg_d['win_length'], hop, cfg_d['n_fft'])
    y = _deemphasis_level(vplan, audio_lib._stft_filter_launch(vplan, x, up.d_lens, gain, d_nuse), d_nuse, Fout, cfg_d, 0.0)
    y, n_samples = _resample_output(y, h_nsamp, d_nsamp, h.res_out, cfg_d, out_sr, res_type)
    return _DIFF_NT(y, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred, gain, [int(v) for v in n_use], f0_src)


# --------------------------------------------------------------------------- time scale (csrc/vc_wsola.hip)
WSOLA_MAX_LEN = 1 << 24     # vc_wsola_plan, vc_wsola_ola_f32: samples per utterance
WSOLA_MAX_FRAMES = 16384    # output frames
WSOLA_MAX_HOP = 1024
WSOLA_MAX_S = 1024          # group * hop_length, the synthesis hop
WSOLA_MAX_TOL = 1024
_PLAN_WSOLA_NT = namedtuple('wsola_plan', 'a cost n_grains out_len hop group tol max_len out_frames')
_SCALE_NT = namedtuple('time_scale', 'y n_samples plan')
_DIFF_DUR_NT = namedtuple('convert_diff_duration', _DIFF_NT._fields + ('flags', 'seg', 'map', 'plan', 'max_frames', 'max_samples',
                                                                       'src_frames'))
_wsola_windows = {}


def wsola_window(S, device=None):
    """The cross-fade table of the time-scale overlap-add (include/vc_hip.h, "Time scale"): T[r] = float32(0.5 - 0.5
    cos(pi r / S)), r = 0 .. S - 1, made in float64.  A numpy array without ``device``; with one, the device's cached copy."""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= S <= WSOLA_MAX_S:
        raise ValueError(' - ERROR, wsola_window: S must be an integer in [1, {}], got {!r}'.format(WSOLA_MAX_S, S))
    S = int(S)
    w = (0.5 - 0.5 * np.cos(np.pi * np.arange(S, dtype=np.float64) / S)).astype(np.float32)
    if device is None:
        return w
    import torch
    key = (str(torch.device(device)), S)
    if key not in _wsola_windows:
        _wsola_windows[key] = torch.from_numpy(w).pin_memory().to(device, non_blocking=True)
    return _wsola_windows[key]


def _check_wsola_args(B, Lmax, Fw, hop, group, tol, qscale, what):
    """(hop, group, tol, qscale) as the launches take them; ValueError beyond their limits."""
    for v, name, hi in ((hop, 'hop_length', WSOLA_MAX_HOP), (group, 'group', WSOLA_MAX_S)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError(' - ERROR, {}: {} must be an integer in [1, {}], got {!r}'.format(what, name, hi, v))
    S = int(group) * int(hop)
    if S > WSOLA_MAX_S:
        raise ValueError(' - ERROR, {}: group * hop_length must be at most {}, got {}'.format(what, WSOLA_MAX_S, S))
    if tol is None:
        tol = S
    if isinstance(tol, bool) or not isinstance(tol, (int, np.integer)) or not 0 <= tol <= WSOLA_MAX_TOL:
        raise ValueError(' - ERROR, {}: tol must be an integer in [0, {}], got {!r}'.format(what, WSOLA_MAX_TOL, tol))
    if isinstance(qscale, bool) or not isinstance(qscale, (int, float, np.integer, np.floating)) \
            or not 0.0 < float(qscale) <= float(np.finfo(np.float32).max) or float(np.float32(qscale)) == 0.0:
        raise ValueError(' - ERROR, {}: qscale must be a positive finite float32, got {!r}'.format(what, qscale))
    if not 1 <= B <= 65535 or not 1 <= Lmax <= WSOLA_MAX_LEN or not 1 <= Fw <= WSOLA_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: 1 to 65535 utterances of 1 to {} samples and 1 to {} output frames (got {} of {} and {})'.format(
            what, WSOLA_MAX_LEN, WSOLA_MAX_FRAMES, B, Lmax, Fw))
    return int(hop), int(group), int(tol), float(qscale)


def _check_count(v, B, hi, what):
    """lens / n_out on the host: B integers in [0, hi]; a device tensor is clamped by the launch."""
    import torch
    if torch.is_tensor(v) and v.is_cuda:
        return
    h = np.asarray(v.cpu() if torch.is_tensor(v) else v)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > hi:
        raise ValueError(' - ERROR, {} must be {} integers in [0, {}]'.format(what, B, hi))


def _wsola_plan_launch(wav, d_lens, pos, d_nout, hop, group, tol, qscale):
    """vc_wsola_plan on validated device tensors: no host check, copy or wait in here."""
    import torch
    import _vc
    lib = _vc.lib()
    B, Lmax = wav.shape
    Fw = pos.shape[1]
    M = lib.vc_wsola_max_grains(Fw, hop, group)
    if M == 0:
        raise _vc.VCError('vc_wsola_max_grains refused {} frames at hop {} and group {}'.format(Fw, hop, group))
    tab = torch.empty((2, B, M), dtype=torch.int32, device=wav.device)
    n = torch.empty((2, B), dtype=torch.int32, device=wav.device)
    _vc.check(lib.vc_wsola_plan(_vc.ptr(wav), Lmax, _vc.ptr(d_lens), _vc.ptr(pos), _vc.ptr(d_nout), B, Lmax, Fw, hop, group, tol, qscale,
                                _vc.ptr(tab[0]), _vc.ptr(tab[1]), _vc.ptr(n[0]), _vc.ptr(n[1]), _vc.current_stream()))
    return _PLAN_WSOLA_NT(tab[0], tab[1], n[0], n[1], hop, group, tol, Lmax, Fw)


def _wsola_ola_launch(wav, d_lens, plan):
    """vc_wsola_ola_f32 on validated device tensors (wav [B, plan.max_len] contiguous float32)."""
    import torch
    import _vc
    B, Lmax = wav.shape
    y = torch.empty((B, plan.hop * (plan.out_frames - 1)), dtype=torch.float32, device=wav.device)
    _vc.check(_vc.lib().vc_wsola_ola_f32(_vc.ptr(wav), Lmax, _vc.ptr(d_lens), _vc.ptr(plan.a), _vc.ptr(plan.n_grains), _vc.ptr(plan.out_len),
                                         _vc.ptr(wsola_window(plan.group * plan.hop, wav.device)), B, Lmax, plan.out_frames, plan.hop,
                                         plan.group, _vc.ptr(y) if y.numel() else None, _vc.current_stream()))
    return y


def _wsola_inputs(what, wav, lens, pos, n_out, hop_length, group, tol, qscale):
    """The checks and uploads that wsola_plan_batch and time_scale_batch share: (wav, d_lens, pos, d_nout, hop, group, tol,
    qscale) on the device; every ValueError before anything is uploaded."""
    import torch
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    if torch.is_tensor(wav) and wav.dtype != torch.float32:
        raise ValueError(' - ERROR, {}: wav must be float32, got {}'.format(what, wav.dtype))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    if getattr(pos, 'ndim', 0) != 2 or pos.shape[0] != B or pos.shape[1] < 1:
        raise ValueError(' - ERROR, {}: pos must be [B, out_frames] with B = {}'.format(what, B))
    Fw = int(pos.shape[1])
    if (pos.dtype != torch.int32) if torch.is_tensor(pos) else (np.asarray(pos).dtype.kind not in 'iu'):
        raise ValueError(' - ERROR, {}: pos must be int32 (Q16 frames), got {}'.format(what, pos.dtype))
    hop, group, tol, qscale = _check_wsola_args(B, Lmax, Fw, hop_length, group, tol, qscale, what)
    if lens is None:
        lens = np.full((B,), Lmax, dtype=np.int64)
    _check_count(lens, B, Lmax, what + ': lens')
    _check_count(n_out, B, Fw, what + ': n_out')
    _need_gpu(what)
    d_pos = _i32_device(pos, (B, Fw), what + ': pos')
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    wsola_window(group * hop, wav.device)
    return wav, _i32_device(lens, (B,), what + ': lens'), d_pos, _i32_device(n_out, (B,), what + ': n_out'), hop, group, tol, qscale


def wsola_plan_batch(wav, lens, pos, n_out, hop_length, group=2, tol=None, qscale=32768.0):
    """The grain plan of time_scale_batch alone (vc_wsola_plan; the definition is in include/vc_hip.h, "Time scale", the numpy
    restatement in tests/wsola_ref.py): for every grain k of an utterance the input sample a_k it is centred on -- within
    ``tol`` samples of where the map points, chosen so that it continues grain k - 1 -- and the cost it was chosen at.

    The arguments are time_scale_batch's.  Returns a namedtuple: the device tensors a, cost [B, M] int32 (INT32_MIN and -1
    from an utterance's grain count on; M = ceil(hop * (out_frames - 1) / S) + 1), n_grains and out_len [B], and the host
    integers hop, group, tol, max_len, out_frames.  Nothing is copied back and the host waits for nothing."""
    wav, d_lens, d_pos, d_nout, hop, group, tol, qscale = _wsola_inputs('wsola_plan_batch', wav, lens, pos, n_out, hop_length, group, tol,
                                                                        qscale)
    return _wsola_plan_launch(wav, d_lens, d_pos, d_nout, hop, group, tol, qscale)


def time_scale_batch(wav, lens, pos, n_out, hop_length, group=2, tol=None, qscale=32768.0):
    """Moves B waveforms along a time map and keeps their pitch and local phase: waveform-similarity overlap-add
    (vc_wsola_plan, vc_wsola_ola_f32).

    wav [B, Lmax] float32 (cuda tensor or numpy array); lens: sample counts, host integers, an int32 [B] device tensor or
    None (all Lmax).  pos [B, out_frames] int32 Q16 input FRAMES and n_out [B] as duration_map_batch returns them (frame u
    is centred on sample u * hop_length); n_out may be host integers too.  group: frames per synthesis hop (S = group *
    hop_length samples; a grain is 2 S long, S <= 1024); tol: the search half width in samples (default S: at 16 kHz and
    hop 80, 10 ms, periods down to 50 Hz); qscale: the factor that takes the samples to 16-bit integers for the similarity
    search (32768 for a waveform within [-1, 1]; larger values clip, smaller ones lose resolution -- the output samples are
    always copied from ``wav`` itself).
    Returns a namedtuple: y [B, hop_length * (out_frames - 1)] float32 on the device (zero from an utterance's length on),
    n_samples [B] (DEVICE int32: hop_length * (n_out - 1)) and plan (wsola_plan_batch's result).  Nothing is copied back and
    the host waits for nothing."""
    wav, d_lens, d_pos, d_nout, hop, group, tol, qscale = _wsola_inputs('time_scale_batch', wav, lens, pos, n_out, hop_length, group, tol,
                                                                        qscale)
    plan = _wsola_plan_launch(wav, d_lens, d_pos, d_nout, hop, group, tol, qscale)
    return _SCALE_NT(_wsola_ola_launch(wav, d_lens, plan), plan.out_len, plan)


def convert_diff_duration_batch(decoder, wav, lens=None, cfg_d=None, rate=None, ratio=None, gap_ratio=1.0, segments='decode',
                                decode=None, out_len=None, max_frames=None, group=2, tol=None, qscale=32768.0, alpha=1.0,
                                max_boost_db=20.0, max_cut_db=30.0, half_width=8, pitch=None, stats_src=None, stats_tgt=None,
                                w_floor=0.5, f0_args=None, t_e=60, two_pass=True, utt_ids=None, window_batch=64, encoder=None,
                                wav_sr=None, out_sr=None, res_type='kaiser_best', denoise=None,
                                dereverb=None):
    """``convert_diff_batch`` with the timing changed as well: the source is filtered exactly as there
    (gain, filter, level, and ``pitch=`` before the filter), then the FILTERED WAVEFORM is moved along an integer time map by
    time_scale_batch -- grains of the natural recording, so its excitation and local phase survive -- and only then
    resampled to out_sr.

    rate / ratio / gap_ratio / segments / decode / out_len / max_frames: convert_duration_batch's, with the map built over
    the n_use = min(n_out, n_clip) frames the filter covers (segments='decode' decodes ``phn_pred`` over those frames) and
    min_frames = 2: an utterance whose table is invalid or whose total would fall below 2 frames keeps its timing (flags
    1, 2).  group, tol, qscale: time_scale_batch's.  The other arguments are convert_diff_batch's, denoise included.
    Returns convert_diff_batch's fields -- y_wav_pred [B, max_samples] at the NEW timing; mel_true / mel_pred / stft_true /
    stft_pred / phn_pred / gain / f0_src stay at the SOURCE's timing -- with n_samples and n_frames as DEVICE tensors (the
    output's; n_samples at out_sr when resampled), plus flags [B], seg = (labels, start, end, n_seg) in output frames, map
    (the duration_map_batch result), plan (the wsola_plan_batch result) and the host bounds max_frames, max_samples and
    src_frames (n_use).  After the uploads nothing is copied to the host and the host waits for nothing."""
    what = 'convert_diff_duration_batch'
    _need_cfg(cfg_d, what)
    req = _duration_request(what, rate, ratio, gap_ratio, segments, decode, out_len)
    h = _convert_host(what, decoder, wav, lens, cfg_d, 0, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr, res_type,
                      denoise, dereverb)
    B, hop, Fout = h.B, h.hop, h.plan.Fout
    n_use, h_nsamp = diff_frames(h.plan, hop)
    req = _duration_bound(what, req, n_use, Fout, 2, max_frames, 'at least {} are needed')
    Fw = req.Fw
    hop, group, tol, qscale = _check_wsola_args(B, hop * (Fout - 1), Fw, hop, group, tol, qscale, what)
    req = _duration_decoder(what, req, decoder, encoder, B, Fout)

    # ---- convert_diff_batch's launches at the model's rate (its own checks run before its first launch), then two tables
    d = convert_diff_batch(decoder, wav, lens=lens, cfg_d=cfg_d, alpha=alpha, max_boost_db=max_boost_db, max_cut_db=max_cut_db,
                           half_width=half_width, pitch=pitch, stats_src=stats_src, stats_tgt=stats_tgt, w_floor=w_floor,
                           f0_args=f0_args, t_e=t_e, two_pass=two_pass, utt_ids=utt_ids, window_batch=window_batch, encoder=encoder,
                           wav_sr=wav_sr, out_sr=None, res_type=res_type, denoise=denoise, dereverb=dereverb)
    d_nuse = _i32_device(n_use, (B,), what + ': n_use')
    d_nsamp = _i32_device(h_nsamp, (B,), what + ': n_samples')
    wsola_window(group * hop, d.y_wav_pred.device)
    m, seg = _duration_map(what, req, d_nuse, d.phn_pred, Fout)   # the segment table in source frames, the map

    # ---- the filtered waveform along the map, the output resampler
    x = d.y_wav_pred.contiguous()
    wplan = _wsola_plan_launch(x, d_nsamp, m.pos, m.n_out, hop, group, tol, qscale)
    y, n_samples, max_samples = _resample_output_device(_wsola_ola_launch(x, d_nsamp, wplan), wplan.out_len, hop * (Fw - 1), h.res_out,
                                                        cfg_d, out_sr, res_type)
    return _DIFF_DUR_NT(y, n_samples, d.mel_true, d.mel_pred, d.stft_true, d.stft_pred, d.phn_pred, d.gain, m.n_out, d.f0_src, m.flags,
                        seg, m, wplan, Fw, max_samples, [int(v) for v in n_use])


# --------------------------------------------------------------------------- postfilter (csrc/vc_postfilter.hip)
_POST_NT = namedtuple('convert_postfilter', _BATCH_NT._fields + ('stft_raw',))


def convert_postfilter_batch(decoder, wav, lens=None, cfg_d=None, model=None, mode='ms', k=0.85, alpha=1.0, max_db=20.0, g_max=4.0,
                             t_s=0, t_e=60, n_iter=200, realse=1.0, two_pass=True, momentum=0.0, phase='device', seed=0,
                             utt_ids=None, window_batch=64, encoder=None, wav_sr=None, out_sr=None, res_type='kaiser_best',
                             denoise=None, dereverb=None):
    """``convert_batch`` with the predicted spectrum postfiltered before the vocoder: the stitched ``stft_pred`` goes through
    postfilter.apply_batch (mode 'ms', 'gv' or 'ms+gv'; k, alpha, max_db, g_max are its arguments) with the frame counts the
    device already holds, then through vc_power_to_amp (``realse`` still applies) and the vocoder.

    model: a postfilter.Model (postfilter.fit on the target speaker's natural spectra and on stft_pred of training
    utterances) or postfilter.upload's device tables -- upload once per model when the call has to stay free of
    host-to-device copies.  The other arguments are convert_batch's; the true spectrum is not vocoded, and phase='numpy'
    is convert_batch's alone.  mel_pred is left as predicted.  denoise: as convert_batch's (mel_true / stft_true are those
    of the denoised input).

    Returns convert_batch's fields (y_wav_true None) plus stft_raw, the spectrum as stitched; stft_pred is the filtered
    one.  With k = 0 and alpha = 0 the filters return their input bit for bit and so does the call: y_wav_pred equals
    convert_batch's.  Nothing is copied to the host and the host waits for nothing.  Nobody has listened to the result
    (DESIGN.md section 28)."""
    import audio_lib
    import postfilter
    what = 'convert_postfilter_batch'
    momentum = _check_momentum(momentum)
    seed = audio_lib.check_seed(seed)
    _need_cfg(cfg_d, what)
    if model is None:
        raise ValueError(' - ERROR, {}: model (postfilter.fit or postfilter.upload) is required'.format(what))
    _check_phase(phase, what)
    postfilter.check_apply_args(mode, k, alpha, max_db, g_max, what)
    h = _convert_host(what, decoder, wav, lens, cfg_d, t_s, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr,
                      res_type, denoise, dereverb)
    plan, Fout, n_bins = h.plan, h.plan.Fout, h.n_bins
    if Fout > postfilter.MAX_FRAMES:
        raise ValueError(' - ERROR, {}: at most {} stitched frames per utterance (got {})'.format(what, postfilter.MAX_FRAMES, Fout))
    _check_phase(phase, what, (h.B, Fout, n_bins))
    _need_gpu(what)
    tables = model if isinstance(model, postfilter.Tables) else postfilter.upload(model, k)
    if tables.gv_t.shape[0] != n_bins:
        raise ValueError(' - ERROR, {}: the model has {} channels, the spectrum {}'.format(what, tables.gv_t.shape[0], n_bins))

    up = _convert_upload(h, wav, [h.h_nsamp] if h.res_out else [])
    phase = _phase_upload(phase)
    mel_true, stft_true, y_mel, y_stft, y_phn = _convert_model(decoder, encoder, h, up, cfg_d, wav_sr, res_type)
    mel_pred, phn_pred, stft_raw, _ = _stitch(y_mel, y_phn, y_stft, up.d_utt, Fout)
    stft_pred = postfilter.apply_batch(stft_raw, up.d_nout, tables, mode=mode, k=k, alpha=alpha, max_db=max_db, g_max=g_max)
    _, y_wav_pred = _vocoder_tail(cfg_d, up.d_nout, up.d_ids, n_iter, momentum, realse, seed, phase, phase, None, stft_pred, None)
    y_wav_pred, n_samples = _resample_output(y_wav_pred, h.h_nsamp, up.d_extra[-1] if h.res_out else None, h.res_out, cfg_d, out_sr,
                                             res_type)
    return _POST_NT(None, y_wav_pred, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred, [int(v) for v in plan.n_out],
                    stft_raw)


# --------------------------------------------------------------------------- spectral mapping (csrc/vc_mapping.hip)
_GMM_DIFF_NT = namedtuple('convert_gmm_diff', 'y_wav_pred n_samples mel_true cep_src cep_pred gain n_frames')


def convert_gmm_diff_batch(model, wav, lens=None, cfg_d=None, mixture='soft', mlpg=True, alpha=1.0, max_boost_db=20.0, max_cut_db=30.0,
                           wav_sr=None, out_sr=None, res_type='kaiser_best', denoise=None, n_coef=None, first_coef=1,
                           dereverb=None):
    """Waveform in, waveform out, with no encoder and no decoder: the source's mel cepstra are
    converted by a joint-density mixture (mapping.fit / mapping.fit_wav; mapping.convert_cepstra_batch with ``mixture`` and
    ``mlpg``), the cepstral difference becomes the gain of the differential filter (mapping.cepstra_gain_batch with alpha,
    max_boost_db, max_cut_db) and the source recording is filtered by it (audio_lib.stft_filter_batch): sprocket's DIFFVC.
    The framing is convert_diff_batch's with every frame used: frame u of the gain is frame u of the source's front-end,
    n_frames = 1 + len // hop per utterance and the output holds hop * (n_frames - 1) samples of it.

    model: a mapping.JDGMM over D = 2 n features; n_coef: None = n.  wav, lens, wav_sr, out_sr, res_type, denoise, dereverb: as
    convert_diff_batch's.  Pitch and durations are not offered here: call pitch_shift_batch / time_scale_batch on the result.
    Returns a namedtuple: y_wav_pred [B, hop * (Fmax - 1)] (the filtered source at the level convert_batch sets, zero beyond
    an utterance's n_samples), n_samples (host, at out_sr when given), mel_true [B, Fmax, n_mels], cep_src and cep_pred
    [B, Fmax, n], gain [B, Fmax, bins] and n_frames (host).  Every check and table is made on the host before the first
    launch; after the uploads nothing is copied to the host and the host waits for nothing."""
    import torch
    import audio_lib
    import evaluation
    import mapping
    what = 'convert_gmm_diff_batch'
    _need_cfg(cfg_d, what)
    alpha, boost, cut = _check_diff_args(alpha, max_boost_db, max_cut_db, what)
    mix = mapping._check_mixture(mixture, what)
    if not (isinstance(model, tuple) and len(model) == 6 and getattr(model[1], 'ndim', 0) == 2):
        raise ValueError(' - ERROR, {}: model must be a mapping.JDGMM'.format(what))
    D = int(model[1].shape[1])
    n = mapping._check_even(D, what)
    if n_coef is not None and int(n_coef) != n:
        raise ValueError(' - ERROR, {}: the model converts {} coefficients, n_coef is {}'.format(what, n, n_coef))
    M = mapping._check_model(model, D, what)
    first_coef = int(first_coef)
    dct, i0, w, scale = mapping._gain_args(cfg_d, n, first_coef, what)
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    hop, sr = int(cfg_d['hop_length']), cfg_d['sample_rate']
    n_fft = cfg_d['n_fft'] or cfg_d['win_length']
    audio_lib._res_params(res_type)
    res_in = wav_sr is not None and audio_lib._ratio(wav_sr, sr) != (1, 1)
    res_out = out_sr is not None and audio_lib._ratio(sr, out_sr) != (1, 1)
    h_lens = np.full((B,), Lmax, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    if h_lens.shape != (B,) or h_lens.min() <= 0 or h_lens.max() > Lmax:
        raise ValueError(' - ERROR, {}: lens must be [B] with 0 < len <= Lmax'.format(what))
    h_lens_in = None
    if res_in:
        h_lens_in, h_lens, Lmax = h_lens, audio_lib.resample_len(h_lens, wav_sr, sr), int(audio_lib.resample_len(Lmax, wav_sr, sr))
    denoise = _check_denoise(what, denoise, cfg_d, B)
    dereverb = _check_dereverb(what, dereverb, cfg_d, Lmax)
    if denoise is not None or dereverb is not None:
        h_lens = hop * (h_lens // hop)
    n_use = 1 + h_lens // hop
    h_nsamp = hop * (n_use - 1)
    if int(h_nsamp.min()) <= n_fft // 2:
        raise ValueError(' - ERROR, {}: every utterance needs hop_length*(frames-1) > n_fft//2 samples at {} Hz'.format(what, sr))
    Fmax = 1 + Lmax // hop
    if B > 65535 or Fmax > mapping.MLPG_MAX_FRAMES:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of at most 2^20 frames'.format(what))
    _need_gpu(what)

    # ---- uploads: the waveforms if they are on the host, one table of lengths, the gain's tables
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    tabs = evaluation._upload_lens(*([h_lens_in] if res_in else []), h_lens, n_use, h_nsamp)
    d_lens, d_nuse, d_nsamp = tabs[-3:]
    d_i0, d_w = mapping._gain_upload(i0, w)
    model = mapping._model_to_device(model)
    h = _HOST_NT(None, B, hop, n_fft, 1 + n_fft // 2, h_lens, h_lens_in, h_nsamp, None, res_in, res_out, None, denoise, dereverb)
    up = _UP_NT(wav, d_lens, None, None, None, None, None, None, tabs[:1])
    h, up = _resample_input(h, up, cfg_d, wav_sr, res_type)
    h, up = _denoise_input(h, up, cfg_d, h.denoise)
    x = up.wav

    # ---- front-end, cepstra, the mapping, gain, filter, level
    mel_true = evaluation._mel_launch(x, d_lens, cfg_d)
    cep_src = evaluation._cepstra_launch(mel_true, n, first_coef)
    cep_pred, _ = mapping._convert_device(model, mapping._prepare_launch(model), cep_src, d_nuse, mix, bool(mlpg))
    gain = mapping._gain_launch(cep_pred, cep_src, d_nuse, evaluation._dct_device(int(cfg_d['n_mels']), n, first_coef), d_i0, d_w, alpha,
                                scale, boost, cut)
    vplan = audio_lib._get_voc_plan(cfg_d['win_length'], hop, cfg_d['n_fft'])
    F = gain.shape[1]
    y = _deemphasis_level(vplan, audio_lib._stft_filter_launch(vplan, x, d_lens, gain, d_nuse), d_nuse, F, cfg_d, 0.0)
    y, n_samples = _resample_output(y, h_nsamp, d_nsamp, res_out, cfg_d, out_sr, res_type)
    return _GMM_DIFF_NT(y, n_samples, mel_true, cep_src, cep_pred, gain, [int(v) for v in n_use])


# --------------------------------------------------------------------------- exemplar conversion (csrc/vc_knn.hip)
_KNN_DIFF_NT = namedtuple('convert_knn_diff', _DIFF_NT._fields + ('idx', 'dist', 'n_used'))


def convert_knn_diff_batch(bank, wav, lens=None, cfg_d=None, encoder=None, ppg=None, k=4, d_max=None, exclude=None, n_splits=0,
                           alpha=1.0, max_boost_db=20.0, max_cut_db=30.0, half_width=8, pitch=None, stats_src=None, stats_tgt=None,
                           w_floor=0.5, f0_args=None, t_e=60, two_pass=True, utt_ids=None, window_batch=64, wav_sr=None, out_sr=None,
                           res_type='kaiser_best', denoise=None, dereverb=None):
    """``convert_diff_batch`` without a decoder: every source frame's spectrum is predicted as the mean
    of the k frames of the target speaker's ``bank`` (exemplar.build_bank / exemplar.bank_wav) whose posteriors are nearest
    to its own, and the source recording is filtered by the difference, as convert_diff_batch filters it.

    Exactly one of encoder (the phoneme recogniser; the windows go through it as in convert_batch) and ppg ([B, Fout, C]
    float32 posteriors that are already there, frame u = front-end frame u) is given; C must be the bank's n_classes.
    k, exclude, n_splits: exemplar.knn_batch's (exclude=bank.rows[...] leaves an utterance's own recording out).  d_max:
    exemplar.mean_batch's.  The mean is taken in the domain of the bank's values, the front-end's normalised dB spectrum
    and mel: a geometric mean of powers.
    Framing, the frames used (n_use = min(n_out, n_clip) of convert_plan with t_s = 0) and every other argument are
    convert_diff_batch's.  Returns its namedtuple -- stft_pred / mel_pred are the retrieved means, phn_pred the posteriors
    that were searched with -- followed by idx, dist [B, Fout, k] and n_used [B, Fout] (int32, on the device; -1 / 0 in
    frames at or beyond n_use).  Every check and table is made on the host before the first launch; after the uploads
    nothing is copied to the host and the host waits for nothing."""
    import torch
    import audio_lib
    import evaluation
    import exemplar
    what = 'convert_knn_diff_batch'
    _need_cfg(cfg_d, what)
    alpha, boost, cut = _check_diff_args(alpha, max_boost_db, max_cut_db, what)
    h_taps = _check_diff_taps(half_width, None, what)
    if hasattr(pitch, 'item') and getattr(pitch, 'ndim', None) == 0:
        pitch = pitch.item()
    kind, pitch = _parse_pitch(pitch, stats_src, stats_tgt, what, True, ('source',),
                               "None, a ratio, a [B, Fout] contour or 'source'", "pitch='source'")
    if kind == 'source' and stats_src is None:
        raise ValueError(" - ERROR, {}: pitch='source' needs stats_src and stats_tgt (the source's own contour unmapped changes nothing)".format(what))
    if kind == 'source' and (len(stats_src) != 3 or len(stats_tgt) != 3):
        raise ValueError(' - ERROR, {}: stats must be (count, mean, std) as f0_stats_batch returns them'.format(what))
    w_floor = _check_w_floor(w_floor, what)
    f0_kw = _tracker_keys(f0_args, what)
    if (encoder is None) == (ppg is None):
        raise ValueError(' - ERROR, {}: pass exactly one of encoder and ppg'.format(what))
    N, Kp = exemplar._check_bank(bank, what)
    k, n_splits = exemplar._check_k(k, what), exemplar._check_splits(n_splits, what)
    d_max = exemplar._check_d_max(d_max, what)
    h = _convert_host(what, None, wav, lens, cfg_d, 0, t_e, two_pass, utt_ids, window_batch, True, encoder, wav_sr, out_sr, res_type,
                      denoise, dereverb, need_decoder=False)
    plan, B, hop, Fout, sr = h.plan, h.B, h.hop, h.plan.Fout, cfg_d['sample_rate']
    C = int(ppg.shape[2]) if ppg is not None and getattr(ppg, 'ndim', 0) == 3 else int(encoder.cfg_d['n_output']) if encoder is not None else 0
    if ppg is not None and evaluation._check_ppg(ppg, what + ': ppg') != (B, Fout, C):
        raise ValueError(' - ERROR, {}: ppg must be [{}, {}, C]'.format(what, B, Fout))
    if C != int(bank.n_classes) or exemplar.key_width(C) != Kp:
        raise ValueError(' - ERROR, {}: the bank was keyed over {} classes, the posteriors hold {}'.format(what, bank.n_classes, C))
    for t, name, width in ((bank.stft, 'stft', h.n_bins), (bank.mel, 'mel', int(cfg_d['n_mels']))):
        if getattr(t, 'ndim', 0) != 2 or tuple(t.shape) != (N, width) or str(t.dtype) not in ('torch.float32', 'float32'):
            raise ValueError(' - ERROR, {}: bank.{} must be float32 [{}, {}]'.format(what, name, N, width))
    if B * Fout > exemplar.MAX_ROWS:
        raise ValueError(' - ERROR, {}: at most 2^24 query frames (got {} x {})'.format(what, B, Fout))
    h_excl = exemplar._check_exclude(exclude, B, N, what)
    n_use, h_nsamp = diff_frames(plan, hop)
    if int(h_nsamp.min()) <= h.n_fft // 2:
        raise ValueError(' - ERROR, {}: every utterance needs hop_length*(frames-1) > n_fft//2 samples'.format(what))
    Lmax = int(audio_lib.resample_len(int(wav.shape[1]), wav_sr, sr)) if h.res_in else int(wav.shape[1])
    if kind is not None:
        tracker = _tracker_args(f0_kw, sr, hop, what)
        _check_pitch_sizes(B, Lmax, 1 + Lmax // hop, hop, what)
        if Lmax > evaluation.F0_MAX_SAMPLES:
            raise ValueError(' - ERROR, {}: the tracker takes at most {} samples per utterance'.format(what, evaluation.F0_MAX_SAMPLES))
        _check_contour(kind, pitch, B, Fout, what, 'frame')
    _need_gpu(what)

    # ---- uploads: the waveforms if they are on the host, one table, the taps, a contour, the posteriors, the bank
    extra = [n_use, h_nsamp, plan.n_src] + ([] if h_excl is None else [h_excl])
    up = _convert_upload(h, wav, extra)
    if up.wav.shape[0] == 1:                                        # (the stride of a one-row tensor is arbitrary)
        up = up._replace(wav=up.wav.as_strided(up.wav.shape, (up.wav.shape[1], 1)))
    d_nuse, d_nsamp, d_fsrc = up.d_extra[-len(extra):][:3]
    d_excl = None if h_excl is None else up.d_extra[-1]
    d_taps = torch.from_numpy(h_taps).pin_memory().to('cuda', non_blocking=True)
    pitch = _contour_upload(kind, pitch)
    if kind is not None:
        psola_window('cuda')
    if ppg is not None:
        ppg = evaluation._to_device(ppg, torch.float32)
    bank = bank._replace(key=exemplar._dev(bank.key, torch.int8), norm=exemplar._dev(bank.norm, torch.int32),
                         stft=exemplar._dev(bank.stft, torch.float32), mel=exemplar._dev(bank.mel, torch.float32))
    h, up = _resample_input(h, up, cfg_d, wav_sr, res_type)
    h, up = _denoise_input(h, up, cfg_d, h.denoise)

    # ---- front-end, windows, the recogniser
    mfcc, mel, pdb = evaluation._fe_launch(up.wav, up.d_lens, cfg_d)
    mel_true = cut_windows(mel, up.d_true, up.d_clip, Fout)
    stft_true = cut_windows(pdb, up.d_true, up.d_clip, Fout)
    if ppg is None:
        win = cut_windows(mfcc, up.d_win, up.d_clip, plan.T)
        ys = [encoder.forward(win[i:i + h.window_batch])['y_pred'] for i in range(0, win.shape[0], h.window_batch)]
        ppg = compound_stitch(ys[0] if len(ys) == 1 else torch.cat(ys, 0), up.d_utt, Fout)

    # ---- keys, search, the two means
    keys, norms = exemplar._key_launch(ppg, d_nuse)
    idx, dist = exemplar._knn_launch(keys, norms, d_nuse, h_excl, d_excl, bank, k, n_splits)
    stft_pred, n_used = exemplar._mean_launch(idx, dist, bank.stft, d_max)
    mel_pred, _ = exemplar._mean_launch(idx, dist, bank.mel, d_max)

    # ---- the source's fundamental, moved before the filter
    x, f0_src = up.wav, None
    if kind is not None:
        f0_src = evaluation._f0_track_launch(x, up.d_lens, d_fsrc, *tracker)[0]
        target = None
        if kind == 'source':
            target = f0_transform(f0_src, stats_src, stats_tgt)
        elif kind == 'contour':
            n = min(Fout, f0_src.shape[1])
            target = torch.zeros_like(f0_src)
            target[:, :n] = pitch[:, :n].to(torch.float32)
        per, rat = pitch_tables(f0_src, sr, ratio=pitch if kind == 'ratio' else None, target_f0=target, hop_length=hop)
        x = _psola_ola_launch(x, up.d_lens, _psola_plan_launch(per, rat, up.d_lens, x.shape[1], hop), w_floor)

    # ---- gain, filter, level
    gain = _diff_gain_launch(stft_pred, stft_true, d_nuse, float(cfg_d['P_dB_norm_factor']), alpha, boost, cut, d_taps)
    vplan = audio_lib._get_voc_plan(cfg_d['win_length'], hop, cfg_d['n_fft'])
    y = _deemphasis_level(vplan, audio_lib._stft_filter_launch(vplan, x, up.d_lens, gain, d_nuse), d_nuse, Fout, cfg_d, 0.0)
    y, n_samples = _resample_output(y, h_nsamp, d_nsamp, h.res_out, cfg_d, out_sr, res_type)
    return _KNN_DIFF_NT(y, n_samples, mel_true, mel_pred, stft_true, stft_pred, ppg, gain, [int(v) for v in n_use], f0_src, idx, dist,
                        n_used)
