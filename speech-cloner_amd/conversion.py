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


def convert_batch(decoder, wav, lens=None, cfg_d=None, t_s=0, t_e=60, n_iter=200, realse=1.0, two_pass=True,
                  giffin_lim_input=False, momentum=0.0, phase='device', seed=0, utt_ids=None, window_batch=64,
                  vocode=True, encoder=None, wav_sr=None, out_sr=None, res_type='kaiser_best'):
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
    Returns a namedtuple of cuda tensors -- y_wav_pred, y_wav_true (None unless giffin_lim_input) [B, hop*(Fout-1)],
    mel_pred / stft_pred / phn_pred and mel_true / stft_true [B, Fout, C], zero beyond an utterance's own extent --
    and the host counts n_frames [B] (= N_b * n_timesteps) and n_samples [B] (= hop * (n_frames - 1)).
    Every check and every table is made on the host from ``lens`` before the first launch; after that nothing is
    copied to the host and the host waits for nothing."""
    import torch
    import audio_lib
    import _vc
    momentum = _check_momentum(momentum)
    seed = audio_lib.check_seed(seed)
    if cfg_d is None:
        raise ValueError(' - ERROR, convert_batch: cfg_d (the data-set configuration) is required')
    if isinstance(phase, str) and phase not in ('device', 'numpy', 'spsi'):
        raise ValueError(" - ERROR, convert_batch: phase must be 'device', 'numpy', 'spsi' or a [B, Fout, bins] array, got {!r}".format(phase))
    if getattr(wav, 'ndim', 0) != 2:
        raise ValueError(' - ERROR, convert_batch: wav must be [B, Lmax]')
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    n_fft = cfg_d['n_fft'] or cfg_d['win_length']
    h_lens = np.full((B,), Lmax, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    sr = cfg_d['sample_rate']
    audio_lib._res_params(res_type)
    res_in = wav_sr is not None and audio_lib._ratio(wav_sr, sr) != (1, 1)
    res_out = vocode and out_sr is not None and audio_lib._ratio(sr, out_sr) != (1, 1)
    if res_in:
        # lens count samples at wav_sr; everything below (checks, tables) works on the resampled lengths
        if h_lens.shape != (B,) or h_lens.min() <= 0 or h_lens.max() > Lmax:
            raise ValueError(' - ERROR, convert_batch: lens must be [B] with 0 < len <= Lmax')
        h_lens_in, Lmax_in = h_lens, Lmax
        h_lens, Lmax = audio_lib.resample_len(h_lens_in, wav_sr, sr), audio_lib.resample_len(Lmax_in, wav_sr, sr)
        if h_lens.min() <= n_fft // 2:
            raise ValueError(' - ERROR, convert_batch: every utterance needs more than n_fft//2 = {} samples at {} Hz '
                             '(shortest: {} after resampling from {} Hz)'.format(n_fft // 2, sr, int(h_lens.min()), wav_sr))
    if h_lens.shape != (B,) or h_lens.min() <= n_fft // 2 or h_lens.max() > Lmax:
        raise ValueError(' - ERROR, convert_batch: lens must be [B] with n_fft//2 < len <= Lmax')
    if utt_ids is None:
        utt_ids = np.arange(B)
    utt_ids = np.asarray(utt_ids, dtype=np.int64).reshape(-1)
    if utt_ids.shape != (B,) or utt_ids.min() < -2 ** 31 or utt_ids.max() >= 2 ** 31:
        raise ValueError(' - ERROR, convert_batch: utt_ids must be {} int32 values, one per utterance'.format(B))
    window_batch = int(window_batch)
    if window_batch <= 0:
        raise ValueError(' - ERROR, convert_batch: window_batch must be positive')
    if (decoder.encoder is None) == (encoder is None):
        raise ValueError(' - ERROR, convert_batch: pass encoder= exactly when the decoder was built without one')
    plan = convert_plan(h_lens, cfg_d, t_s, t_e, two_pass)
    hop, T, Fout = int(cfg_d['hop_length']), plan.T, plan.Fout
    n_bins = 1 + n_fft // 2
    if vocode and hop * (int(plan.n_out.min()) - 1) <= n_fft // 2:
        raise ValueError(' - ERROR, convert_batch: every utterance needs hop_length*(frames-1) > n_fft//2 samples')
    both = bool(giffin_lim_input)
    h_phase = None
    if not isinstance(phase, str):
        if tuple(phase.shape) != (B, Fout, n_bins):
            raise ValueError(' - ERROR, convert_batch: phase must be [{}, {}, {}]'.format(B, Fout, n_bins))
    if not torch.cuda.is_available():
        raise _vc.VCError('convert_batch needs a GPU (no CPU fallback)')

    # ---- uploads: the waveforms if they are on the host, one table, the host-drawn phase if asked for
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    parts = [h_lens, plan.n_clip, plan.n_out, utt_ids, plan.win_tab, plan.utt_tab, plan.true_tab]
    h_nsamp = hop * (plan.n_out.astype(np.int64) - 1)
    if res_in:
        parts.append(h_lens_in)
    if res_out:
        parts.append(h_nsamp)
    h_tab = torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1) for a in parts])).pin_memory()
    d_tab = h_tab.to('cuda', non_blocking=True)
    offs = np.cumsum([0] + [a.size for a in parts])
    d_lens, d_clip, d_nout, d_ids, d_win, d_utt, d_true = (d_tab[offs[i]:offs[i + 1]] for i in range(7))
    d_extra = [d_tab[offs[i]:offs[i + 1]] for i in range(7, len(parts))]
    d_win, d_utt, d_true = d_win.view(-1, 2), d_utt.view(-1, 3), d_true.view(-1, 2)
    if vocode and isinstance(phase, str) and phase == 'numpy':
        h_phase = torch.from_numpy(_numpy_phase(plan, n_bins, both)).pin_memory()
        d_phase = h_phase.to('cuda', non_blocking=True)
        ph_true, ph_pred = d_phase[0], d_phase[-1]
    elif vocode and not isinstance(phase, str):
        if not torch.is_tensor(phase):
            phase = torch.from_numpy(np.ascontiguousarray(phase, dtype=np.float32))
        ph_true = ph_pred = phase.to(device='cuda', dtype=torch.float32).contiguous()

    # ---- front-end, windows, model, stitch
    if res_in:
        wav = audio_lib._resample_launch(audio_lib._get_res_plan(wav_sr, sr, res_type), wav, d_extra[0])
    mfcc, mel, pdb = audio_lib.calc_MFCC_input_batch(
        wav, d_lens, sr=cfg_d['sample_rate'], pre_emphasis=cfg_d['pre_emphasis'], hop_length=hop,
        win_length=cfg_d['win_length'], n_mels=cfg_d['n_mels'], n_mfcc=cfg_d['n_mfcc'], n_fft=cfg_d['n_fft'],
        window=cfg_d['window'], mfcc_normaleze_first_mfcc=cfg_d['mfcc_normaleze_first_mfcc'],
        mfcc_norm_factor=cfg_d['mfcc_norm_factor'], calc_mfcc_derivate=cfg_d['calc_mfcc_derivate'],
        M_dB_norm_factor=cfg_d['M_dB_norm_factor'], P_dB_norm_factor=cfg_d['P_dB_norm_factor'],
        mean_abs_amp_norm=cfg_d['mean_abs_amp_norm'], clip_output=cfg_d['clip_output'])
    x = cut_windows(mfcc, d_win, d_clip, T)
    mel_true = cut_windows(mel, d_true, d_clip, Fout)
    stft_true = cut_windows(pdb, d_true, d_clip, Fout)
    if encoder is None:
        outs = decoder.forward_chunks(x, window_batch, n_streams=2)
    else:
        outs = decoder.forward_chunks(x, window_batch, n_streams=2, width=x.shape[2],
                                      fn=lambda xb: decoder.forward(encoder.forward(xb)['y_pred']))
    main = torch.cuda.current_stream()
    cols = []
    for key in ('y_mel', 'y_stft', 'y_phn'):
        ts = [o[key] for o in outs]
        for t in ts:
            t.record_stream(main)
        cols.append(ts[0] if len(ts) == 1 else torch.cat(ts, 0))
    y_mel, y_stft, y_phn = cols
    mel_pred = compound_stitch(y_mel, d_utt, Fout)
    phn_pred = compound_stitch(y_phn, d_utt, Fout)
    fused = vocode and float(realse) == 1.0
    if fused:
        stft_pred, amp_pred = compound_stitch(y_stft, d_utt, Fout, P_dB_norm_factor=cfg_d['P_dB_norm_factor'])
    else:
        stft_pred = compound_stitch(y_stft, d_utt, Fout)
    n_frames = [int(v) for v in plan.n_out]
    n_samples = [int(v) for v in h_nsamp]
    if not vocode:
        return _BATCH_NT(None, None, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred, n_frames)

    # ---- vocoder
    vplan = audio_lib._get_voc_plan(cfg_d['win_length'], hop, cfg_d['n_fft'])
    lib = _vc.lib()
    if isinstance(phase, str) and phase == 'device':
        ph_true = ph_pred = audio_lib.phase_init(d_nout, Fout, n_bins, seed, d_ids)
    elif isinstance(phase, str) and phase == 'spsi':
        ph_true = ph_pred = None                                   # from each spectrum's own magnitudes, in to_wav

    def power_to_amp(P, rl):
        amp = torch.empty_like(P)
        _vc.check(lib.vc_power_to_amp(_vc.ptr(P), _vc.ptr(d_nout), B, Fout, n_bins, float(cfg_d['P_dB_norm_factor']),
                                      float(rl), _vc.ptr(amp), _vc.current_stream()))
        return amp

    def to_wav(amp, ph):
        if ph is None:
            ph = audio_lib._phase_spsi_launch(amp, d_nout, vplan.n_fft, vplan.hop_length, plan=vplan)
        w = audio_lib._griffin_lim_launch(vplan, amp, ph, d_nout, n_iter, False, momentum)
        _vc.check(lib.vc_inv_preemphasis_normalize(vplan.handle, _vc.ptr(w), _vc.ptr(d_nout), B, Fout, w.shape[1],
                                                   float(cfg_d['pre_emphasis']), float(15 * cfg_d['mean_abs_amp_norm']),
                                                   _vc.current_stream()))
        return w

    y_wav_true = to_wav(power_to_amp(stft_true, 1.0), ph_true) if both else None
    y_wav_pred = to_wav(amp_pred if fused else power_to_amp(stft_pred, realse), ph_pred)
    if res_out:
        rplan = audio_lib._get_res_plan(sr, out_sr, res_type)
        y_wav_pred = audio_lib._resample_launch(rplan, y_wav_pred, d_extra[-1])
        if both:
            y_wav_true = audio_lib._resample_launch(rplan, y_wav_true, d_extra[-1])
        n_samples = [int(v) for v in audio_lib.resample_len(h_nsamp, sr, out_sr)]
    return _BATCH_NT(y_wav_true, y_wav_pred, n_samples, mel_true, mel_pred, stft_true, stft_pred, phn_pred, n_frames)
