"""Signal front-end with the reference's ``audio_lib`` surface, computed on the MI355X.

Mirrors /root/reference/audio_lib.py: same function names, argument order, defaults and
return types for the functions on the conversion hot path:

  calc_MFCC_input(y, ...) -> (MFCC [F, n_mfcc*(1|2)], M_dB [F, n_mels], P_dB [F, 1+n_fft//2])
                              np.float32, time-major, F = 1 + len(y)//hop_length
                              (audio_lib.py:89-244)
  calc_preemphasis / calc_inv_preemphasis                      (audio_lib.py:12-47)
  calc_PHN_target                                              (audio_lib.py:51-85)
  griffin_lim_alg(stft_amp [bins, F], ...) -> wav              (audio_lib.py:249-274)
  from_power_to_wav(P [F, bins], ...) -> wav                   (audio_lib.py:278-308)

plus batched entry points the reference does not have (its per-utterance calls are special
cases of them):

  calc_MFCC_input_batch(wav [B, L], lens=None, ...) -> three torch.cuda tensors [B, Fmax, C]
  from_power_to_wav_batch(P [B, Fmax, bins], n_frames=None, ...) -> torch.cuda tensor [B, hop*(Fmax-1)]
  phase_init(n_frames, Fmax, n_bins, seed, utt_ids) -> torch.cuda tensor [B, Fmax, bins], Griffin-Lim's initial
                              phase drawn on the device (Philox4x32-10; include/vc_hip.h vc_phase_init);
                              the batched vocoder calls take it as ``phase0='device'``
  phase_spsi(amp, n_frames)  -> torch.cuda tensor [B, Fmax, bins], a deterministic initial phase computed from the
                             magnitudes (single-pass spectrogram inversion; include/vc_hip.h vc_phase_spsi);
                             the batched vocoder calls take it as ``phase0='spsi'``
  stft_filter_batch(wav, lens, gain, n_frames) -> torch.cuda tensor [B, hop*(F-1)]: istft(gain * stft(wav)), one
                             transform pass that keeps the input's phase (include/vc_hip.h vc_stft_filter_f32)

  envelope_batch / hnm_plan_batch / noise_batch / hnm_synth_batch: the harmonic-plus-noise vocoder -- a spectral envelope
                             and an F0 contour in, a waveform out, no phase iteration (include/vc_hip.h,
                             "Harmonic-plus-noise vocoder")

The Griffin-Lim entry points take ``momentum`` (default 0.0, the reference's algorithm): fast
Griffin-Lim as in librosa.griffinlim / torchaudio GriffinLim, see include/vc_hip.h
vc_griffin_lim_momentum_f32.

All arithmetic runs in hand-written HIP kernels (csrc/vc_frontend.hip) through the C ABI
``vc_frontend_f32`` (include/vc_hip.h); torch only owns the device buffers.  There is no
CPU path: without the native library or a GPU the calls raise.
"""
import collections
import ctypes as C
import math

import numpy as np

import _vc

_PLANS = {}


class _Plan:
    def __init__(self, cfg, window):
        from scipy import signal
        lib = _vc.lib()
        self.cfg = cfg
        if isinstance(window, str) or isinstance(window, tuple):
            w = signal.get_window(window, cfg.win_length, fftbins=True)
        else:
            w = np.asarray(window, dtype=np.float64)
            if w.shape != (cfg.win_length,):
                raise ValueError(' - ERROR, window array must have win_length samples')
        self._w = np.ascontiguousarray(w, dtype=np.float64)
        h = C.c_void_p()
        _vc.check(lib.vc_frontend_plan_create(C.byref(cfg), _vc.ptr(self._w), C.byref(h)))
        self.handle = h
        self.mfcc_width = lib.vc_frontend_mfcc_width(h)
        self.n_bins = lib.vc_frontend_power_width(h)

    def workspace(self, batch, max_samples, device):
        """Scratch for ONE call, from the caching allocator of the current stream: calls of this plan on other
        streams (or in a captured graph) each get their own."""
        import torch
        need = _vc.lib().vc_frontend_workspace_bytes(self.handle, batch, max_samples)
        return torch.empty(need, dtype=torch.uint8, device=device)


def _get_plan(sr, pre_emphasis, hop_length, win_length, n_mels, n_mfcc, n_fft, window,
              mfcc_normaleze_first_mfcc, mfcc_norm_factor, calc_mfcc_derivate,
              M_dB_norm_factor, P_dB_norm_factor, mean_abs_amp_norm, clip_output):
    if n_fft is None:
        n_fft = win_length
    wkey = window if isinstance(window, (str, tuple)) else np.asarray(window).tobytes()
    key = (sr, pre_emphasis, hop_length, win_length, n_mels, n_mfcc, n_fft, wkey,
           bool(mfcc_normaleze_first_mfcc), mfcc_norm_factor, bool(calc_mfcc_derivate),
           M_dB_norm_factor, P_dB_norm_factor, mean_abs_amp_norm, bool(clip_output))
    p = _PLANS.get(key)
    if p is None:
        cfg = _vc.FrontendCfg(int(sr), int(hop_length), int(win_length), int(n_fft), int(n_mels),
                              int(n_mfcc), float(pre_emphasis), float(mean_abs_amp_norm),
                              float(mfcc_norm_factor), float(M_dB_norm_factor),
                              float(P_dB_norm_factor), int(bool(mfcc_normaleze_first_mfcc)),
                              int(bool(calc_mfcc_derivate)), int(bool(clip_output)))
        p = _Plan(cfg, window)
        _PLANS[key] = p
    return p


def calc_MFCC_input_batch(wav, lens=None,
                          sr=16000,
                          pre_emphasis=0.97,
                          hop_length=40,
                          win_length=400,
                          n_mels=128,
                          n_mfcc=40,
                          n_fft=None,
                          window='hann',
                          mfcc_normaleze_first_mfcc=True,
                          mfcc_norm_factor=0.01,
                          calc_mfcc_derivate=False,
                          M_dB_norm_factor=0.01,
                          P_dB_norm_factor=0.01,
                          mean_abs_amp_norm=0.003,
                          clip_output=True,
                          out=None,
                          stage_mask=7,
                          out_frames=None):
    """Batched calc_MFCC_input on the GPU.

    wav  : float32 [B, L] torch.cuda tensor (or numpy array, uploaded).
    lens : optional per-utterance sample counts (sequence / int32 tensor); None = all L.
    out  : optional (mfcc, mel, pow) preallocated cuda tensors to write into.
    stage_mask : measurement hook (bench.py): subset of the three launches, see vc_hip.h.
    out_frames : store only the first out_frames frames of every utterance (the later ones still count for its
                 normalisation statistics): with out_frames a multiple of the window length the result reshapes to the
                 encoder's window batch without a copy.  None = all Fmax = 1 + L//hop_length frames.
    Returns (MFCC [B, R, W], M_dB [B, R, n_mels], P_dB [B, R, 1+n_fft//2]) cuda float32, R = out_frames or Fmax;
    rows beyond an utterance's own frame count are zero."""
    import torch
    if not torch.cuda.is_available():
        raise _vc.VCError('calc_MFCC_input needs a GPU (no CPU fallback)')
    plan = _get_plan(sr, pre_emphasis, hop_length, win_length, n_mels, n_mfcc, n_fft, window,
                     mfcc_normaleze_first_mfcc, mfcc_norm_factor, calc_mfcc_derivate,
                     M_dB_norm_factor, P_dB_norm_factor, mean_abs_amp_norm, clip_output)
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    if wav.dim() != 2:
        raise ValueError(' - ERROR, calc_MFCC_input_batch: wav must be [B, L]')
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    B, L = wav.shape
    half = plan.cfg.n_fft // 2
    d_lens = None
    if lens is not None:
        if torch.is_tensor(lens):
            d_lens = lens.to(device='cuda', dtype=torch.int32).contiguous()
        else:
            h = np.asarray(lens, dtype=np.int32)
            if h.shape != (B,) or h.min() <= half or h.max() > L:
                raise ValueError(' - ERROR, calc_MFCC_input_batch: lens must be [B] with n_fft//2 < len <= L')
            d_lens = torch.from_numpy(h).to('cuda')
    Fmax = 1 + L // plan.cfg.hop_length
    R = Fmax if out_frames is None else int(out_frames)
    if not 0 < R <= Fmax:
        raise ValueError(' - ERROR, calc_MFCC_input_batch: out_frames must be in [1, {}]'.format(Fmax))
    if out is None:
        mfcc = torch.empty((B, R, plan.mfcc_width), dtype=torch.float32, device=wav.device)
        mel = torch.empty((B, R, plan.cfg.n_mels), dtype=torch.float32, device=wav.device)
        pdb = torch.empty((B, R, plan.n_bins), dtype=torch.float32, device=wav.device)
    else:
        mfcc, mel, pdb = out
        for t, w in ((mfcc, plan.mfcc_width), (mel, plan.cfg.n_mels), (pdb, plan.n_bins)):
            if tuple(t.shape) != (B, R, w) or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError(' - ERROR, calc_MFCC_input_batch: out tensors must be contiguous float32 [B, {}, width]'.format(R))
    ws = plan.workspace(B, L, wav.device)
    _vc.check(_vc.lib().vc_frontend_stages_f32(plan.handle, _vc.ptr(wav), _vc.ptr(d_lens), B, L, wav.stride(0), R,
                                               _vc.ptr(mfcc), _vc.ptr(mel), _vc.ptr(pdb),
                                               _vc.ptr(ws), ws.numel(), _vc.current_stream(),
                                               int(stage_mask)))
    return mfcc, mel, pdb


def calc_MFCC_input(y,
                    sr=16000,
                    pre_emphasis=0.97,
                    hop_length=40,
                    win_length=400,
                    n_mels=128,
                    n_mfcc=40,
                    n_fft=None,
                    window='hann',
                    mfcc_normaleze_first_mfcc=True,
                    mfcc_norm_factor=0.01,
                    calc_mfcc_derivate=False,
                    M_dB_norm_factor=0.01,
                    P_dB_norm_factor=0.01,
                    mean_abs_amp_norm=0.003,
                    clip_output=True):
    """Drop-in for audio_lib.calc_MFCC_input (audio_lib.py:89-244): one utterance in (numpy
    1-D array), three np.float32 arrays out, time-major."""
    y = np.ascontiguousarray(np.asarray(y).reshape(1, -1), dtype=np.float32)
    mfcc, mel, pdb = calc_MFCC_input_batch(
        y, None, sr, pre_emphasis, hop_length, win_length, n_mels, n_mfcc, n_fft, window,
        mfcc_normaleze_first_mfcc, mfcc_norm_factor, calc_mfcc_derivate, M_dB_norm_factor,
        P_dB_norm_factor, mean_abs_amp_norm, clip_output)
    return mfcc[0].cpu().numpy(), mel[0].cpu().numpy(), pdb[0].cpu().numpy()


def host_tables(sr, n_fft, n_mels, n_mfcc):
    """(mel [n_mels, 1+n_fft//2], dct [n_mfcc, n_mels]) float64 as the native library builds them
    (host-only; works without a GPU)."""
    cfg = _vc.FrontendCfg(int(sr), 1, int(n_fft), int(n_fft), int(n_mels), int(n_mfcc),
                          0.0, 1.0, 1.0, 1.0, 1.0, 0, 0, 0)
    mel = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float64)
    dct = np.zeros((n_mfcc, n_mels), dtype=np.float64)
    _vc.check(_vc.lib().vc_frontend_host_tables(C.byref(cfg), _vc.ptr(mel), _vc.ptr(dct)))
    return mel, dct


def calc_preemphasis(wav, coeff=0.97):
    """audio_lib.py:12-28 -- y[n] = x[n] - coeff*x[n-1], zero initial state.  Host helper (the
    GPU path fuses this filter into the STFT gather)."""
    wav = np.asarray(wav, dtype=np.float64)
    out = wav.copy()
    out[1:] -= coeff * wav[:-1]
    return out


def calc_inv_preemphasis(preem_wav, coeff=0.97):
    """audio_lib.py:31-47 -- inverse IIR  y[n] = x[n] + coeff*y[n-1]."""
    from scipy import signal
    return signal.lfilter([1], [1, -coeff], preem_wav)


def calc_PHN_target(y, phn_v, phn_conv_d, hop_length=40, win_length=400):
    """audio_lib.py:51-85 -- per-frame phoneme target by larger window overlap (integer host
    logic used when building training caches)."""
    n_samples = int(y.shape[0] / hop_length) + 1
    half_n_fft = win_length // 2
    target_v = []
    i_phn = 0
    for i_s in range(n_samples):
        i_win_s = i_s * hop_length - half_n_fft
        i_win_e = i_win_s + win_length
        while phn_v[i_phn][1] <= i_win_s and i_phn + 1 < len(phn_v):
            i_phn += 1
        cur = phn_v[i_phn]
        pick = cur
        if i_phn + 1 < len(phn_v):
            nxt = phn_v[i_phn + 1]
            d_cur = min(cur[1], i_win_e) - max(cur[0], i_win_s)
            d_nxt = min(nxt[1], i_win_e) - max(nxt[0], i_win_s)
            if d_cur < d_nxt:
                pick = nxt
        target_v.append(phn_conv_d[pick[2]])
    return np.array(target_v, dtype=np.int32)


# --------------------------------------------------------------------------- vocoder
_VOC_PLANS = {}


class _VocPlan:
    def __init__(self, win_length, hop_length, n_fft):
        h = C.c_void_p()
        _vc.check(_vc.lib().vc_vocoder_plan_create(int(win_length), int(hop_length), int(n_fft), None, C.byref(h)))
        self.handle = h
        self.win_length, self.hop_length, self.n_fft = int(win_length), int(hop_length), int(n_fft)
        self.n_bins = 1 + self.n_fft // 2

    def workspace(self, batch, max_frames, trace, device, momentum=False):
        """Scratch for ONE call, from the caching allocator of the current stream (see _Plan.workspace)."""
        import torch
        lib = _vc.lib()
        size = lib.vc_vocoder_workspace_bytes_momentum if momentum else lib.vc_vocoder_workspace_bytes
        return torch.empty(size(self.handle, batch, max_frames, int(trace)), dtype=torch.uint8, device=device)

    def spsi_workspace(self, batch, max_frames, device):
        """Scratch for ONE vc_phase_spsi call at this plan's bins, like workspace()."""
        return _spsi_workspace(batch, max_frames, self.n_bins, device)

    def window_sums(self):
        """(sum w, sum w^2) of the plan's window as the device holds it (float32 values of the periodic Hann window, summed
        in float64): what calibrates the harmonic-plus-noise vocoder."""
        i = np.arange(self.win_length)
        w = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / self.win_length)).astype(np.float32).astype(np.float64)
        return float(w.sum()), float((w * w).sum())


def check_momentum(momentum):
    """Fast Griffin-Lim momentum as a float; ValueError unless finite and in [0, 1) (torchaudio's rule)."""
    m = float(momentum)
    if not (math.isfinite(m) and 0.0 <= m < 1.0):
        raise ValueError(' - ERROR, griffin_lim: momentum must be finite and in [0, 1), got {!r}'.format(momentum))
    return m


def _get_voc_plan(win_length, hop_length, n_fft):
    if n_fft is None:
        n_fft = win_length
    key = (int(win_length), int(hop_length), int(n_fft))
    p = _VOC_PLANS.get(key)
    if p is None:
        p = _VOC_PLANS[key] = _VocPlan(*key)
    return p


def _frames_arg(n_frames, B, Fmax, plan):
    """Validates per-utterance frame counts; returns (device int32 tensor or None, host array)."""
    import torch
    if n_frames is None:
        h = np.full((B,), Fmax, dtype=np.int32)
        d = None
    else:
        h = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames, dtype=np.int32)
        if h.shape != (B,) or h.max() > Fmax:
            raise ValueError(' - ERROR, n_frames must be [B] with values <= {}'.format(Fmax))
        d = torch.from_numpy(h).to('cuda')
    if plan.hop_length * (int(h.min()) - 1) <= plan.n_fft // 2:
        raise ValueError(' - ERROR, griffin_lim: every utterance needs hop_length*(frames-1) > n_fft//2 samples '
                         '(librosa.stft reflect padding)')
    return d, h


def _int32_device(v, n, what):
    """int32 [n] on the device from a host sequence or a tensor (a cuda tensor is used as it is: no copy, no wait)."""
    import torch
    if torch.is_tensor(v):
        if tuple(v.shape) != (n,):
            raise ValueError(' - ERROR, {} must have {} entries'.format(what, n))
        return v.to(device='cuda', dtype=torch.int32).contiguous()
    h = np.asarray(v, dtype=np.int64)
    if h.shape != (n,) or h.min() < -2 ** 31 or h.max() >= 2 ** 31:
        raise ValueError(' - ERROR, {} must be {} int32 values'.format(what, n))
    return torch.from_numpy(h.astype(np.int32)).to('cuda')


def check_seed(seed):
    s = int(seed)
    if not 0 <= s < 2 ** 64:
        raise ValueError(' - ERROR, seed must be in [0, 2**64), got {!r}'.format(seed))
    return s


def phase_init(n_frames, Fmax, n_bins, seed=0, utt_ids=None, out=None):
    """Griffin-Lim's initial phase on the device (vc_phase_init, include/vc_hip.h): float32 [B, Fmax, n_bins] cuda,
    phase[b, f, k] = float32(pi) * U[0, 1) for f < n_frames[b] and 0 beyond, from Philox4x32-10 addressed by
    (seed, utt_ids[b], f * n_bins + k) -- an utterance's phase does not depend on its place in the batch, on Fmax or on
    the other utterances.  n_frames: [B] host ints or int32 cuda tensor; utt_ids likewise (default 0 .. B-1)."""
    import torch
    seed = check_seed(seed)
    B = int(n_frames.shape[0]) if torch.is_tensor(n_frames) else len(n_frames)
    if utt_ids is not None and (int(utt_ids.shape[0]) if torch.is_tensor(utt_ids) else len(utt_ids)) != B:
        raise ValueError(' - ERROR, phase_init: utt_ids must have one entry per utterance ({})'.format(B))
    if not torch.is_tensor(n_frames) and (B == 0 or max(n_frames) > Fmax or min(n_frames) < 0):
        raise ValueError(' - ERROR, phase_init: n_frames must be [B] with values in [0, {}]'.format(Fmax))
    if not torch.cuda.is_available():
        raise _vc.VCError('phase_init needs a GPU (no CPU fallback)')
    d_nf = _int32_device(n_frames, B, 'n_frames')
    d_id = None if utt_ids is None else _int32_device(utt_ids, B, 'utt_ids')
    if out is None:
        out = torch.empty((B, int(Fmax), int(n_bins)), dtype=torch.float32, device='cuda')
    elif tuple(out.shape) != (B, int(Fmax), int(n_bins)) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(' - ERROR, phase_init: out must be contiguous float32 [B, Fmax, n_bins]')
    _vc.check(_vc.lib().vc_phase_init(_vc.ptr(d_nf), _vc.ptr(d_id), B, int(Fmax), int(n_bins),
                                      seed - 2 ** 64 if seed >= 2 ** 63 else seed, _vc.ptr(out),
                                      _vc.current_stream()))
    return out


SPSI_CHUNK_FRAMES = 32          # frames per chunk of vc_phase_spsi's scan (csrc/vc_spsi.hip SPSI_CHUNK)


def _spsi_workspace(batch, max_frames, n_bins, device):
    """Scratch for ONE vc_phase_spsi call, from the caching allocator of the current stream (see _Plan.workspace)."""
    import torch
    return torch.empty(_vc.lib().vc_phase_spsi_workspace_bytes(batch, max_frames, n_bins), dtype=torch.uint8, device=device)


def _phase_spsi_launch(amp, d_nf, n_fft, hop_length, out=None, plan=None):
    """The launches of phase_spsi on validated device tensors (amp [B, Fmax, 1 + n_fft//2] float32 contiguous, d_nf int32
    [B] or None): no host check, copy or wait in here.  plan: the vocoder plan that hands out the scratch (the vocoder
    calls pass theirs; phase_spsi on its own needs none, so it also takes sizes a vocoder plan does not)."""
    import torch
    B, Fmax, nb = amp.shape
    if out is None:
        out = torch.empty_like(amp)
    ws = plan.spsi_workspace(B, Fmax, amp.device) if plan is not None else _spsi_workspace(B, Fmax, nb, amp.device)
    _vc.check(_vc.lib().vc_phase_spsi(_vc.ptr(amp), _vc.ptr(d_nf), B, Fmax, nb, int(n_fft), int(hop_length), _vc.ptr(out),
                                      _vc.ptr(ws), ws.numel(), _vc.current_stream()))
    return out


def phase_spsi(amp, n_frames=None, hop_length=80, n_fft=400, out=None):
    """A deterministic initial phase for Griffin-Lim from the magnitudes alone (vc_phase_spsi, include/vc_hip.h): float32
    [B, Fmax, bins] cuda.  Single-pass spectrogram inversion: every frame's spectral peaks advance by hop_length times
    their interpolated frequency and lock their neighbouring bins; rows beyond n_frames are 0.  amp: float32
    [B, Fmax, 1 + n_fft//2] magnitudes, frame-major (numpy or tensor; expected finite and non-negative).  n_frames: [B]
    host ints or int32 cuda tensor (None = all Fmax).  No seed and no utt_ids: an utterance's phase depends on its own
    magnitudes only, not on its place in the batch, on Fmax or on the other utterances."""
    import torch
    n_fft, hop_length = int(n_fft), int(hop_length)
    if not torch.is_tensor(amp):
        amp = torch.from_numpy(np.ascontiguousarray(amp, dtype=np.float32))
    if amp.dim() != 3 or amp.shape[0] == 0 or amp.shape[1] == 0 or amp.shape[2] != 1 + n_fft // 2:
        raise ValueError(' - ERROR, phase_spsi: amp must be [B, F, {}]'.format(1 + n_fft // 2))
    B, Fmax, nb = (int(v) for v in amp.shape)
    if n_frames is not None:
        if (int(n_frames.shape[0]) if torch.is_tensor(n_frames) else len(n_frames)) != B:
            raise ValueError(' - ERROR, phase_spsi: n_frames must have one entry per utterance ({})'.format(B))
        if not torch.is_tensor(n_frames) and (max(n_frames) > Fmax or min(n_frames) < 0):
            raise ValueError(' - ERROR, phase_spsi: n_frames must be [B] with values in [0, {}]'.format(Fmax))
    if not torch.cuda.is_available():
        raise _vc.VCError('phase_spsi needs a GPU (no CPU fallback)')
    amp = amp.to(device='cuda', dtype=torch.float32).contiguous()
    d_nf = None if n_frames is None else _int32_device(n_frames, B, 'n_frames')
    if out is not None and (tuple(out.shape) != (B, Fmax, nb) or out.dtype != torch.float32 or not out.is_contiguous()
                            or not out.is_cuda):
        raise ValueError(' - ERROR, phase_spsi: out must be contiguous cuda float32 [B, Fmax, bins]')
    return _phase_spsi_launch(amp, d_nf, n_fft, hop_length, out)


def _check_phase0_name(phase0):
    if isinstance(phase0, str) and phase0 not in ('device', 'spsi'):
        raise ValueError(" - ERROR, griffin_lim_batch: phase0 must be None, 'device', 'spsi' or an array, got {!r}".format(phase0))


def _griffin_lim_launch(plan, amp, phase0, d_nf, num_iters, trace, momentum):
    """The launches of griffin_lim_batch on validated device tensors (amp, phase0 [B, Fmax, bins] float32 contiguous,
    d_nf int32 [B] or None): no host check, copy or wait in here."""
    import torch
    B, Fmax, _ = amp.shape
    L = plan.hop_length * (Fmax - 1)
    wav = torch.empty((B, L), dtype=torch.float32, device=amp.device)
    tr = torch.empty((int(num_iters), B), dtype=torch.float32, device=amp.device) if trace else None
    ws = plan.workspace(B, Fmax, trace, amp.device, momentum=momentum > 0.0)
    if momentum == 0.0:
        _vc.check(_vc.lib().vc_griffin_lim_f32(plan.handle, _vc.ptr(amp), _vc.ptr(phase0), _vc.ptr(d_nf), B, Fmax,
                                               int(num_iters), _vc.ptr(wav), L, _vc.ptr(tr), _vc.ptr(ws), ws.numel(),
                                               _vc.current_stream()))
    else:
        _vc.check(_vc.lib().vc_griffin_lim_momentum_f32(plan.handle, _vc.ptr(amp), _vc.ptr(phase0), _vc.ptr(d_nf), B,
                                                        Fmax, int(num_iters), momentum, _vc.ptr(wav), L, _vc.ptr(tr),
                                                        _vc.ptr(ws), ws.numel(), _vc.current_stream()))
    return (wav, tr) if trace else wav


def griffin_lim_batch(amp, n_frames=None, win_length=400, hop_length=80, num_iters=300, n_fft=None, phase0=None,
                      trace=False, momentum=0.0, seed=0, utt_ids=None):
    """Batched Griffin-Lim on the GPU.  amp: float32 [B, Fmax, bins] magnitudes (frame-major, the
    decoder's y_stft layout); phase0: same shape, radians (default: pi * np.random.rand drawn per
    utterance in the reference's [bins, F] order, audio_lib.py:255), or 'device': drawn by
    phase_init(n_frames, Fmax, bins, seed, utt_ids) without touching the host generator, or 'spsi': computed from amp by
    phase_spsi (deterministic; seed and utt_ids are not used).  momentum: fast Griffin-Lim
    (0 <= momentum < 1; 0 = the reference's algorithm, 0.99 = librosa's default).
    Returns wav [B, hop*(Fmax-1)] cuda float32 (zero beyond an utterance's hop*(frames-1) samples)
    and, with ``trace``, the per-iteration sum of squared waveform changes [num_iters, B]."""
    import torch
    momentum = check_momentum(momentum)
    _check_phase0_name(phase0)
    if not torch.cuda.is_available():
        raise _vc.VCError('griffin_lim needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(win_length, hop_length, n_fft)
    if not torch.is_tensor(amp):
        amp = torch.from_numpy(np.ascontiguousarray(amp, dtype=np.float32))
    amp = amp.to(device='cuda', dtype=torch.float32).contiguous()
    if amp.dim() != 3 or amp.shape[2] != plan.n_bins:
        raise ValueError(' - ERROR, griffin_lim_batch: amp must be [B, F, {}]'.format(plan.n_bins))
    B, Fmax, nb = amp.shape
    d_nf, h_nf = _frames_arg(n_frames, B, Fmax, plan)
    if isinstance(phase0, str):
        if phase0 == 'spsi':
            phase0 = _phase_spsi_launch(amp, d_nf, plan.n_fft, plan.hop_length, plan=plan)
        else:
            phase0 = phase_init(h_nf if d_nf is None else d_nf, Fmax, nb, seed, utt_ids)
    elif phase0 is None:
        ph = np.zeros((B, Fmax, nb), dtype=np.float32)
        for b in range(B):
            ph[b, :h_nf[b]] = (np.pi * np.random.rand(nb, int(h_nf[b]))).T
        phase0 = torch.from_numpy(ph)
    elif not torch.is_tensor(phase0):
        phase0 = torch.from_numpy(np.ascontiguousarray(phase0, dtype=np.float32))
    phase0 = phase0.to(device='cuda', dtype=torch.float32).contiguous()
    if phase0.shape != amp.shape:
        raise ValueError(' - ERROR, griffin_lim_batch: phase0 must have the shape of amp')
    return _griffin_lim_launch(plan, amp, phase0, d_nf, num_iters, trace, momentum)


def _stft_filter_launch(plan, wav, d_len, gain, d_nf):
    """vc_stft_filter_f32 on validated device tensors (wav [B, Lmax], gain [B, Fmax, bins] float32 contiguous, d_len int32
    [B], d_nf int32 [B] or None): no host check, copy or wait in here."""
    import torch
    B, Fmax, _ = gain.shape
    L = plan.hop_length * (Fmax - 1)
    out = torch.empty((B, L), dtype=torch.float32, device=wav.device)
    ws = torch.empty(_vc.lib().vc_stft_filter_workspace_bytes(plan.handle, B, Fmax), dtype=torch.uint8, device=wav.device)
    _vc.check(_vc.lib().vc_stft_filter_f32(plan.handle, _vc.ptr(wav), wav.shape[1], _vc.ptr(d_len), _vc.ptr(gain), _vc.ptr(d_nf), B,
                                           Fmax, _vc.ptr(out), L, _vc.ptr(ws), ws.numel(), _vc.current_stream()))
    return out


def stft_filter_batch(wav, lens, gain, n_frames=None, win_length=400, hop_length=80, n_fft=None):
    """y = istft(gain * stft(wav)) for a ragged batch, in librosa's sense (vc_stft_filter_f32, include/vc_hip.h,
    "Differential-spectrum conversion"): one transform pass, the source's own phase.

    wav [B, Lmax] float32 (numpy or tensor); lens: the sample counts, host integers or an int32 [B] device tensor (None =
    all Lmax); gain [B, F, 1 + n_fft//2] float32, real (zero-phase; the filtering is circular within a frame); n_frames:
    the frames to use per utterance, host integers or an int32 [B] device tensor (None = 1 + len // hop_length); in every
    case at most F and at most 1 + len // hop_length are used.
    Returns y [B, hop_length * (F - 1)] float32 on the device: hop_length * (frames - 1) samples per utterance, zeros
    beyond; an utterance shorter than the reflect padding (len <= n_fft//2, or hop_length * (frames - 1) <= n_fft//2) gives a
    row of zeros.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'stft_filter_batch'
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    plan_key = (int(win_length), int(hop_length), int(n_fft or win_length))
    nb = 1 + plan_key[2] // 2
    if getattr(gain, 'ndim', 0) != 3 or gain.shape[0] != B or gain.shape[1] < 2 or gain.shape[2] != nb:
        raise ValueError(' - ERROR, {}: gain must be [{}, F, {}] with F >= 2'.format(what, B, nb))
    if B > 65535:
        raise ValueError(' - ERROR, {}: at most 65535 utterances'.format(what))
    for v, hi, name in ((lens, Lmax, 'lens'), (n_frames, int(gain.shape[1]), 'n_frames')):
        if v is None or (torch.is_tensor(v) and v.is_cuda):
            if v is not None and (v.dtype != torch.int32 or tuple(v.shape) != (B,)):
                raise ValueError(' - ERROR, {}: {} on the device must be int32 [{}]'.format(what, name, B))
            continue
        h = np.asarray(v.cpu() if torch.is_tensor(v) else v)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > hi:
            raise ValueError(' - ERROR, {}: {} must be {} integers in [0, {}]'.format(what, name, B, hi))
    if not torch.cuda.is_available():
        raise _vc.VCError('stft_filter_batch needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(*plan_key)
    as_dev = lambda t: (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))).to(
        device='cuda', dtype=torch.float32).contiguous()
    d_len = _int32_device(np.full((B,), Lmax, np.int64) if lens is None else lens, B, 'lens')
    d_nf = None if n_frames is None else _int32_device(n_frames, B, 'n_frames')
    return _stft_filter_launch(plan, as_dev(wav), d_len, as_dev(gain), d_nf)


def _stft_power_launch(plan, wav, d_len, d_nf, Fmax):
    """vc_stft_power_f32 on validated device tensors (wav [B, Lmax] float32 contiguous, d_len int32 [B], d_nf int32 [B] or
    None): (power [B, Fmax, bins], the frame counts the device used, int32 [B]); no host check, copy or wait in here."""
    import torch
    B = wav.shape[0]
    power = torch.empty((B, Fmax, plan.n_bins), dtype=torch.float32, device=wav.device)
    d_fout = torch.empty((B,), dtype=torch.int32, device=wav.device)
    _vc.check(_vc.lib().vc_stft_power_f32(plan.handle, _vc.ptr(wav), wav.shape[1], _vc.ptr(d_len), _vc.ptr(d_nf), B, Fmax,
                                          _vc.ptr(power), _vc.ptr(d_fout), _vc.current_stream()))
    return power, d_fout


def _check_stft_wave_args(what, wav, lens, n_frames, win_length, hop_length, n_fft):
    """The host checks stft_power_batch and enhance.denoise_batch share, in stft_filter_batch's style: (B, Lmax, Fmax, plan key).
    Fmax = 1 + Lmax // hop_length; ValueError before the GPU is touched."""
    import torch
    if getattr(wav, 'ndim', 0) != 2 or min(wav.shape) < 1:
        raise ValueError(' - ERROR, {}: wav must be [B, Lmax]'.format(what))
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    for v, name in ((win_length, 'win_length'), (hop_length, 'hop_length')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(' - ERROR, {}: {} must be a positive integer, got {!r}'.format(what, name, v))
    if n_fft is not None and (isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or n_fft < win_length):
        raise ValueError(' - ERROR, {}: n_fft must be None or an integer >= win_length, got {!r}'.format(what, n_fft))
    plan_key = (int(win_length), int(hop_length), int(n_fft or win_length))
    if plan_key[2] % 2 or plan_key[2] > 4096 or plan_key[1] > plan_key[2]:
        raise ValueError(' - ERROR, {}: need n_fft even, n_fft <= 4096 and hop_length <= n_fft (got {}, {})'.format(
            what, plan_key[2], plan_key[1]))
    if B > 65535:
        raise ValueError(' - ERROR, {}: at most 65535 utterances'.format(what))
    Fmax = 1 + Lmax // plan_key[1]
    for v, hi, name in ((lens, Lmax, 'lens'), (n_frames, Fmax, 'n_frames')):
        if v is None or (torch.is_tensor(v) and v.is_cuda):
            if v is not None and (v.dtype != torch.int32 or tuple(v.shape) != (B,)):
                raise ValueError(' - ERROR, {}: {} on the device must be int32 [{}]'.format(what, name, B))
            continue
        h = np.asarray(v.cpu() if torch.is_tensor(v) else v)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > hi:
            raise ValueError(' - ERROR, {}: {} must be {} integers in [0, {}]'.format(what, name, B, hi))
    return B, Lmax, Fmax, plan_key


def _stft_wave_upload(wav, lens, n_frames, B, Lmax):
    """(wav float32 contiguous, d_len int32 [B], d_nf int32 [B] or None) on the device, after _check_stft_wave_args."""
    import torch
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32).contiguous()
    d_len = _int32_device(np.full((B,), Lmax, np.int64) if lens is None else lens, B, 'lens')
    d_nf = None if n_frames is None else _int32_device(n_frames, B, 'n_frames')
    return wav, d_len, d_nf


def stft_power_batch(wav, lens, n_frames=None, win_length=400, hop_length=80, n_fft=None):
    """P = |stft(wav)|^2, linear and unnormalised, for a ragged batch (vc_stft_power_f32, include/vc_hip.h, "Noise
    suppression"): exactly the frames stft_filter_batch transforms -- the same window, reflect padding and frame counts.

    wav [B, Lmax] float32 (numpy or tensor); lens: the sample counts, host integers or an int32 [B] device tensor (None =
    all Lmax); n_frames: the frames to use per utterance, host integers or an int32 [B] device tensor (None = 1 + len //
    hop_length); in every case at most 1 + len // hop_length are used.
    Returns (power [B, 1 + Lmax // hop_length, 1 + n_fft//2] float32, n_frames_device int32 [B]), both on the device: rows
    at or beyond an utterance's frame count are 0, and an utterance shorter than the reflect padding (len <= n_fft//2, or
    hop_length * (frames - 1) <= n_fft//2) has the count 0.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'stft_power_batch'
    B, Lmax, Fmax, plan_key = _check_stft_wave_args(what, wav, lens, n_frames, win_length, hop_length, n_fft)
    if not torch.cuda.is_available():
        raise _vc.VCError('stft_power_batch needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(*plan_key)
    wav, d_len, d_nf = _stft_wave_upload(wav, lens, n_frames, B, Lmax)
    return _stft_power_launch(plan, wav, d_len, d_nf, Fmax)


def _stft_complex_launch(plan, wav, d_len, d_nf, Fmax):
    """vc_stft_complex_f32 on validated device tensors (as _stft_power_launch): (re, im [B, bins, Fmax], the frame counts the
    device used, int32 [B]); no host check, copy or wait in here."""
    import torch
    B = wav.shape[0]
    re = torch.empty((B, plan.n_bins, Fmax), dtype=torch.float32, device=wav.device)
    im = torch.empty_like(re)
    d_fout = torch.empty((B,), dtype=torch.int32, device=wav.device)
    _vc.check(_vc.lib().vc_stft_complex_f32(plan.handle, _vc.ptr(wav), wav.shape[1], _vc.ptr(d_len), _vc.ptr(d_nf), B, Fmax,
                                            _vc.ptr(re), _vc.ptr(im), _vc.ptr(d_fout), _vc.current_stream()))
    return re, im, d_fout


def stft_complex_batch(wav, lens, n_frames=None, win_length=400, hop_length=80, n_fft=None):
    """Z = stft(wav) for a ragged batch (vc_stft_complex_f32, include/vc_hip.h, "Dereverberation"): exactly the frames
    stft_filter_batch and stft_power_batch transform -- the same window, reflect padding and frame counts.

    wav, lens, n_frames: as stft_power_batch's.  Returns (re, im, n_frames_device): the spectrum planar and BIN-MAJOR, two
    float32 tensors [B, 1 + n_fft//2, 1 + Lmax // hop_length], and int32 [B], all on the device; frames at or beyond an
    utterance's count are 0, and an utterance shorter than the reflect padding has the count 0.  Nothing is copied back and
    the host waits for nothing."""
    import torch
    what = 'stft_complex_batch'
    B, Lmax, Fmax, plan_key = _check_stft_wave_args(what, wav, lens, n_frames, win_length, hop_length, n_fft)
    if not torch.cuda.is_available():
        raise _vc.VCError('stft_complex_batch needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(*plan_key)
    wav, d_len, d_nf = _stft_wave_upload(wav, lens, n_frames, B, Lmax)
    return _stft_complex_launch(plan, wav, d_len, d_nf, Fmax)


def _istft_complex_launch(plan, re, im, d_nf):
    """vc_istft_complex_f32 on validated device tensors (re, im [B, bins, Fmax] float32 contiguous, d_nf int32 [B] or None):
    y [B, hop * (Fmax - 1)]; no host check, copy or wait in here."""
    import torch
    B, _, Fmax = re.shape
    L = plan.hop_length * (Fmax - 1)
    out = torch.empty((B, L), dtype=torch.float32, device=re.device)
    ws = torch.empty(_vc.lib().vc_stft_filter_workspace_bytes(plan.handle, B, Fmax), dtype=torch.uint8, device=re.device)
    _vc.check(_vc.lib().vc_istft_complex_f32(plan.handle, _vc.ptr(re), _vc.ptr(im), _vc.ptr(d_nf), B, Fmax, _vc.ptr(out), L,
                                             _vc.ptr(ws), ws.numel(), _vc.current_stream()))
    return out


def _check_spectrum_args(what, re, im, n_frames, n_bins=None):
    """The host checks of a planar bin-major spectrum and its frame counts: (B, bins, F).  ValueError before the GPU is
    touched."""
    import torch
    if getattr(re, 'ndim', 0) != 3 or getattr(im, 'ndim', 0) != 3 or tuple(re.shape) != tuple(im.shape) or min(re.shape) < 1:
        raise ValueError(' - ERROR, {}: re and im must be [B, bins, F], of one shape'.format(what))
    B, nb, Fmax = (int(v) for v in re.shape)
    if not 2 <= nb <= 2049 or (n_bins is not None and nb != n_bins):
        raise ValueError(' - ERROR, {}: re and im must hold {} bins, got {}'.format(
            what, 'between 2 and 2049' if n_bins is None else n_bins, nb))
    if B > 65535:
        raise ValueError(' - ERROR, {}: at most 65535 utterances'.format(what))
    if n_frames is not None and torch.is_tensor(n_frames) and n_frames.is_cuda:
        if n_frames.dtype != torch.int32 or tuple(n_frames.shape) != (B,):
            raise ValueError(' - ERROR, {}: n_frames on the device must be int32 [{}]'.format(what, B))
    elif n_frames is not None:
        h = np.asarray(n_frames.cpu() if torch.is_tensor(n_frames) else n_frames)
        if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > Fmax:
            raise ValueError(' - ERROR, {}: n_frames must be {} integers in [0, {}]'.format(what, B, Fmax))
    return B, nb, Fmax


def _spectrum_upload(t):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device='cuda', dtype=torch.float32).contiguous()


def istft_complex_batch(re, im, n_frames, win_length=400, hop_length=80, n_fft=None):
    """y = istft(re + i im) for a ragged batch, in librosa's sense (vc_istft_complex_f32): the inverse of stft_complex_batch.

    re, im [B, 1 + n_fft//2, F] float32, F >= 2 (numpy or tensor); n_frames: host integers or an int32 [B] device tensor
    (None = all F).  The imaginary parts of bin 0 and bin n_fft//2 are ignored.  Returns y [B, hop_length * (F - 1)] float32
    on the device: hop_length * (frames - 1) samples per utterance, zeros beyond; a row of zeros where hop_length *
    (frames - 1) <= n_fft//2.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'istft_complex_batch'
    for v, name in ((win_length, 'win_length'), (hop_length, 'hop_length')):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(' - ERROR, {}: {} must be a positive integer, got {!r}'.format(what, name, v))
    if n_fft is not None and (isinstance(n_fft, bool) or not isinstance(n_fft, (int, np.integer)) or n_fft < win_length):
        raise ValueError(' - ERROR, {}: n_fft must be None or an integer >= win_length, got {!r}'.format(what, n_fft))
    plan_key = (int(win_length), int(hop_length), int(n_fft or win_length))
    if plan_key[2] % 2 or plan_key[2] > 4096 or plan_key[1] > plan_key[2]:
        raise ValueError(' - ERROR, {}: need n_fft even, n_fft <= 4096 and hop_length <= n_fft (got {}, {})'.format(
            what, plan_key[2], plan_key[1]))
    B, _, Fmax = _check_spectrum_args(what, re, im, n_frames, 1 + plan_key[2] // 2)
    if Fmax < 2:
        raise ValueError(' - ERROR, {}: re and im must hold at least 2 frames'.format(what))
    if not torch.cuda.is_available():
        raise _vc.VCError('istft_complex_batch needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(*plan_key)
    d_nf = None if n_frames is None else _int32_device(n_frames, B, 'n_frames')
    return _istft_complex_launch(plan, _spectrum_upload(re), _spectrum_upload(im), d_nf)


# --------------------------------------------------------------------------- harmonic-plus-noise vocoder
HnmPlan = collections.namedtuple('HnmPlan', 'voiced inc slope phase flags')
HnmSynth = collections.namedtuple('HnmSynth', 'y env_log theta plan gain')
_ENV_TABLES = {}


def _env_table(n_fft):
    """float32 [n_fft, 2] on the device: (cos, sin)(2 pi m / n_fft), made in float64 (vc_env_cepstral_f32's table)."""
    import torch
    t = _ENV_TABLES.get(n_fft)
    if t is None:
        m = np.arange(n_fft)
        h = np.stack([np.cos(2.0 * np.pi * m / n_fft), np.sin(2.0 * np.pi * m / n_fft)], axis=1).astype(np.float32)
        t = _ENV_TABLES[n_fft] = torch.from_numpy(h).to('cuda')
    return t


def _hnm_count(v, B, hi, what, name):
    """Host check of a per-utterance count (host integers, an int32 [B] device tensor or None)."""
    import torch
    if v is None:
        return
    if torch.is_tensor(v) and v.is_cuda:
        if v.dtype != torch.int32 or tuple(v.shape) != (B,):
            raise ValueError(' - ERROR, {}: {} on the device must be int32 [{}]'.format(what, name, B))
        return
    h = np.asarray(v.cpu() if torch.is_tensor(v) else v)
    if h.shape != (B,) or h.dtype.kind not in 'iu' or h.min() < 0 or h.max() > hi:
        raise ValueError(' - ERROR, {}: {} must be {} integers in [0, {}]'.format(what, name, B, hi))


def _hnm_float(v, what, name, lo=None, positive=False):
    f = float(v)
    if not math.isfinite(f) or (positive and f <= 0.0) or (lo is not None and f < lo):
        raise ValueError(' - ERROR, {}: {} must be finite{}, got {!r}'.format(
            what, name, ' and positive' if positive else '' if lo is None else ' and at least {}'.format(lo), v))
    return f


def _check_envelope_args(what, shape, n_fft, order, iters, floor):
    n_fft, order, iters = int(n_fft), int(order), int(iters)
    if n_fft < 4 or n_fft % 2 or n_fft > 2048:
        raise ValueError(' - ERROR, {}: n_fft must be even and in [4, 2048], got {}'.format(what, n_fft))
    if len(shape) != 3 or min(shape) < 1 or shape[2] != 1 + n_fft // 2:
        raise ValueError(' - ERROR, {}: amp must be [B, F, {}]'.format(what, 1 + n_fft // 2))
    if shape[0] > 65535 or shape[1] > 16384:
        raise ValueError(' - ERROR, {}: at most 65535 utterances of 16384 frames'.format(what))
    if not 1 <= order < n_fft // 2:
        raise ValueError(' - ERROR, {}: order must be in [1, {}), got {}'.format(what, n_fft // 2, order))
    if not 0 <= iters <= 1024:
        raise ValueError(' - ERROR, {}: iters must be in [0, 1024], got {}'.format(what, iters))
    return n_fft, order, iters, _hnm_float(floor, what, 'floor', positive=True)


def _as_cuda_f32(t):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    return t.to(device='cuda', dtype=torch.float32).contiguous()


def _envelope_launch(amp, d_nf, n_fft, order, iters, floor):
    import torch
    B, F, _ = amp.shape
    env_log, theta = torch.empty_like(amp), torch.empty_like(amp)
    _vc.check(_vc.lib().vc_env_cepstral_f32(_vc.ptr(amp), _vc.ptr(d_nf), _vc.ptr(_env_table(n_fft)), B, F, n_fft, order, iters,
                                            floor, _vc.ptr(env_log), _vc.ptr(theta), _vc.current_stream()))
    return env_log, theta


def envelope_batch(amp, n_frames=None, n_fft=400, order=24, iters=16, floor=1e-5):
    """Spectral envelope and its minimum phase from magnitudes (vc_env_cepstral_f32, include/vc_hip.h): the true-envelope
    iteration on a cepstrum of ``order`` coefficients.  amp [B, F, 1 + n_fft//2] float32 linear magnitudes; n_frames host
    integers or an int32 [B] device tensor (None = all F).  Returns (env_log, theta), float32 [B, F, bins] on the device:
    the natural log of the envelope and its minimum phase in radians; rows beyond n_frames are 0."""
    import torch
    what = 'envelope_batch'
    n_fft, order, iters, floor = _check_envelope_args(what, tuple(getattr(amp, 'shape', ())), n_fft, order, iters, floor)
    B, F = int(amp.shape[0]), int(amp.shape[1])
    _hnm_count(n_frames, B, F, what, 'n_frames')
    if not torch.cuda.is_available():
        raise _vc.VCError('envelope_batch needs a GPU (no CPU fallback)')
    d_nf = None if n_frames is None else _int32_device(n_frames, B, 'n_frames')
    return _envelope_launch(_as_cuda_f32(amp), d_nf, n_fft, order, iters, floor)


def _check_plan_args(what, shape, sr, hop_length, f0_lo, f0_hi):
    sr, hop_length = int(sr), int(hop_length)
    if len(shape) != 2 or min(shape) < 1 or shape[0] > 65535 or shape[1] > 16384:
        raise ValueError(' - ERROR, {}: f0 must be [B, F] with B <= 65535 and F <= 16384'.format(what))
    if sr < 1 or not 1 <= hop_length <= 4096:
        raise ValueError(' - ERROR, {}: need sr >= 1 and hop_length in [1, 4096], got {}, {}'.format(what, sr, hop_length))
    f0_lo = _hnm_float(f0_lo, what, 'f0_lo', positive=True)
    f0_hi = _hnm_float(sr / 4.0 if f0_hi is None else f0_hi, what, 'f0_hi', positive=True)
    if not f0_lo <= f0_hi <= sr / 2.0:
        raise ValueError(' - ERROR, {}: need f0_lo <= f0_hi <= sr / 2, got {}, {}'.format(what, f0_lo, f0_hi))
    return sr, hop_length, f0_lo, f0_hi


def _hnm_plan_launch(f0, d_nf, sr, hop_length, f0_lo, f0_hi):
    import torch
    B, F = f0.shape
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=f0.device)
    pl = HnmPlan(torch.empty((B, F), dtype=torch.uint8, device=f0.device), i32(B, F), i32(B, F), i32(B, F), i32(B))
    _vc.check(_vc.lib().vc_hnm_plan(_vc.ptr(f0), _vc.ptr(d_nf), B, F, sr, hop_length, f0_lo, f0_hi, _vc.ptr(pl.voiced),
                                    _vc.ptr(pl.inc), _vc.ptr(pl.slope), _vc.ptr(pl.phase), _vc.ptr(pl.flags),
                                    _vc.current_stream()))
    return pl


def hnm_plan_batch(f0, n_frames, sr, hop_length, f0_lo=40.0, f0_hi=None):
    """The integer phase track of an F0 contour (vc_hnm_plan, include/vc_hip.h).  f0 [B, F] float32 Hz, 0 = unvoiced;
    n_frames host integers, an int32 [B] device tensor or None; f0_hi defaults to sr / 4.  Returns HnmPlan(voiced uint8
    [B, F], inc, slope, phase int32 [B, F] -- inc and phase hold uint32 bit patterns -- and flags int32 [B], bit 0: some
    non-zero f0 lay outside the limits and counted as unvoiced), all on the device."""
    import torch
    what = 'hnm_plan_batch'
    sr, hop_length, f0_lo, f0_hi = _check_plan_args(what, tuple(getattr(f0, 'shape', ())), sr, hop_length, f0_lo, f0_hi)
    B, F = int(f0.shape[0]), int(f0.shape[1])
    _hnm_count(n_frames, B, F, what, 'n_frames')
    if not torch.cuda.is_available():
        raise _vc.VCError('hnm_plan_batch needs a GPU (no CPU fallback)')
    d_nf = None if n_frames is None else _int32_device(n_frames, B, 'n_frames')
    return _hnm_plan_launch(_as_cuda_f32(f0), d_nf, sr, hop_length, f0_lo, f0_hi)


def _noise_launch(d_lens, B, Lmax, seed, d_id):
    import torch
    out = torch.empty((B, Lmax), dtype=torch.float32, device='cuda')
    _vc.check(_vc.lib().vc_noise_init_f32(_vc.ptr(d_lens), _vc.ptr(d_id), B, Lmax, seed - 2 ** 64 if seed >= 2 ** 63 else seed,
                                          _vc.ptr(out), _vc.current_stream()))
    return out


def noise_batch(lens, Lmax, seed=0, utt_ids=None):
    """Unit-variance uniform noise on the device (vc_noise_init_f32, include/vc_hip.h): float32 [B, Lmax],
    sqrt(12) * (U - 1/2) with U from Philox4x32-10 addressed by (seed, utt_ids[b], sample) as phase_init addresses its
    elements -- an utterance's noise does not depend on the batch or on Lmax.  Zero from lens[b] on.  lens: host integers or
    an int32 [B] device tensor; utt_ids likewise (default 0 .. B-1)."""
    import torch
    what = 'noise_batch'
    seed, Lmax = check_seed(seed), int(Lmax)
    B = int(lens.shape[0]) if torch.is_tensor(lens) else len(lens)
    if B < 1 or B > 65535 or Lmax < 1:
        raise ValueError(' - ERROR, {}: need 1 <= B <= 65535 and Lmax >= 1'.format(what))
    _hnm_count(lens, B, Lmax, what, 'lens')
    if utt_ids is not None and (int(utt_ids.shape[0]) if torch.is_tensor(utt_ids) else len(utt_ids)) != B:
        raise ValueError(' - ERROR, {}: utt_ids must have one entry per utterance ({})'.format(what, B))
    if not torch.cuda.is_available():
        raise _vc.VCError('noise_batch needs a GPU (no CPU fallback)')
    d_id = None if utt_ids is None else _int32_device(utt_ids, B, 'utt_ids')
    return _noise_launch(_int32_device(lens, B, 'lens'), B, Lmax, seed, d_id)


def hnm_cutoff(voiced_cutoff_hz, sr, n_fft, f0_lo):
    """(cutoff_inc, cutoff_bin) of a voiced cutoff in Hz: the phase advance per sample in units of 2^-32 turn (at most 2^31,
    Nyquist) and the first bin at or above the cutoff.  ValueError when cutoff / f0_lo exceeds the harmonic cap (256)."""
    what = 'hnm_synth_batch'
    c = _hnm_float(voiced_cutoff_hz, what, 'voiced_cutoff_hz', positive=True)
    c = min(c, sr / 2.0)
    if c / f0_lo > 256:
        raise ValueError(' - ERROR, {}: voiced_cutoff_hz / f0_lo = {:.1f} exceeds the 256 harmonics a frame can hold'.format(
            what, c / f0_lo))
    return max(1, min(int(round(c * 2.0 ** 32 / sr)), 2 ** 31)), int(math.ceil(c * n_fft / sr))


def _hnm_synth_launch(plan, env_log, theta, pl, d_nf, cutoff_inc, add):
    import torch
    B, F, _ = env_log.shape
    y = torch.empty((B, plan.hop_length * (F - 1)), dtype=torch.float32, device=env_log.device)
    _vc.check(_vc.lib().vc_hnm_synth_f32(_vc.ptr(env_log), _vc.ptr(theta), _vc.ptr(pl.voiced), _vc.ptr(pl.inc), _vc.ptr(pl.slope),
                                         _vc.ptr(pl.phase), _vc.ptr(d_nf), _vc.ptr(add), B, F, plan.n_fft, plan.hop_length,
                                         cutoff_inc, 2.0 / plan.window_sums()[0], _vc.ptr(y), _vc.current_stream()))
    return y


def _hnm_noise_launch(plan, env_log, pl, d_nf, d_lens, cutoff_bin, noise_level, seed, d_id):
    """The noise branch on device tensors: the gain, the noise, and the existing vc_stft_filter_f32 launch.  (filtered, gain)."""
    import torch
    B, F, nb = env_log.shape
    gain = torch.empty_like(env_log)
    _vc.check(_vc.lib().vc_hnm_noise_gain_f32(_vc.ptr(env_log), _vc.ptr(pl.voiced), _vc.ptr(d_nf), B, F, nb, cutoff_bin,
                                              noise_level / math.sqrt(plan.window_sums()[1]), _vc.ptr(gain),
                                              _vc.current_stream()))
    noise = _noise_launch(d_lens, B, plan.hop_length * (F - 1), seed, d_id)
    return _stft_filter_launch(plan, noise, d_lens, gain, d_nf), gain


def _hnm_chain(plan, amp, f0, d_nf, d_lens, sr, order, iters, floor, f0_lo, f0_hi, cutoff, noise_level, seed, d_id, noise):
    """Every launch of hnm_synth_batch on validated device tensors: no host check, copy or wait in here."""
    env_log, theta = _envelope_launch(amp, d_nf, plan.n_fft, order, iters, floor)
    pl = _hnm_plan_launch(f0, d_nf, sr, plan.hop_length, f0_lo, f0_hi)
    add = gain = None
    if noise:
        add, gain = _hnm_noise_launch(plan, env_log, pl, d_nf, d_lens, cutoff[1], noise_level, seed, d_id)
    return HnmSynth(_hnm_synth_launch(plan, env_log, theta, pl, d_nf, cutoff[0], add), env_log, theta, pl, gain)


def hnm_synth_batch(amp, f0, n_frames=None, sr=16000, win_length=400, hop_length=80, n_fft=None, order=24, iters=16,
                    floor=1e-5, voiced_cutoff_hz=4000.0, noise_level=1.0, seed=0, utt_ids=None, noise=True, f0_lo=40.0,
                    f0_hi=None):
    """The harmonic-plus-noise vocoder (include/vc_hip.h): magnitudes and an F0 contour in, a waveform out, one pass.

    amp [B, F, 1 + n_fft//2] float32 linear magnitudes (the envelope is estimated from them: envelope_batch); f0 [B, F]
    float32 Hz, 0 = unvoiced; n_frames host integers or an int32 [B] device tensor (None = all F).  Voiced frames get
    harmonics of f0 below voiced_cutoff_hz, with the envelope's minimum phase, at 2 / sum(w) times the envelope -- the
    magnitude an STFT with the plan's window reads back; unvoiced frames, and voiced ones above the cutoff, get noise
    (noise_batch(seed, utt_ids)) shaped by stft_filter_batch's launch to noise_level times the envelope; noise=False
    leaves it out.  Returns HnmSynth(y [B, hop_length * (F - 1)], env_log, theta, plan, gain), all on the device; y is zero
    beyond hop_length * (n_frames - 1) samples.  Nothing is copied back and the host waits for nothing."""
    import torch
    what = 'hnm_synth_batch'
    win_length = int(win_length)
    n_fft_ = int(n_fft or win_length)
    shape = tuple(getattr(amp, 'shape', ()))
    n_fft_, order, iters, floor = _check_envelope_args(what, shape, n_fft_, order, iters, floor)
    B, F = int(shape[0]), int(shape[1])
    if tuple(getattr(f0, 'shape', ())) != (B, F) or F < 2:
        raise ValueError(' - ERROR, {}: f0 must be [{}, {}] with at least 2 frames'.format(what, B, F))
    sr, hop_length, f0_lo, f0_hi = _check_plan_args(what, (B, F), sr, hop_length, f0_lo, f0_hi)
    if not 1 <= win_length <= n_fft_ or hop_length > n_fft_:
        raise ValueError(' - ERROR, {}: need win_length <= n_fft and hop_length <= n_fft'.format(what))
    cutoff = hnm_cutoff(voiced_cutoff_hz, sr, n_fft_, f0_lo)
    noise_level = _hnm_float(noise_level, what, 'noise_level', lo=0.0)
    seed = check_seed(seed)
    _hnm_count(n_frames, B, F, what, 'n_frames')
    if utt_ids is not None and (int(utt_ids.shape[0]) if torch.is_tensor(utt_ids) else len(utt_ids)) != B:
        raise ValueError(' - ERROR, {}: utt_ids must have one entry per utterance ({})'.format(what, B))
    if not torch.cuda.is_available():
        raise _vc.VCError('hnm_synth_batch needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(win_length, hop_length, n_fft_)
    d_nf = _int32_device(np.full((B,), F, np.int64) if n_frames is None else n_frames, B, 'n_frames')
    d_lens = (d_nf - 1).clamp_(min=0).mul_(hop_length) if noise else None
    d_id = None if utt_ids is None else _int32_device(utt_ids, B, 'utt_ids')
    return _hnm_chain(plan, _as_cuda_f32(amp), _as_cuda_f32(f0), d_nf, d_lens, sr, order, iters, floor, f0_lo, f0_hi, cutoff,
                      noise_level, seed, d_id, bool(noise))


def griffin_lim_alg(stft_amp, win_length, hop_length, num_iters=300, n_fft=None, verbose=True, phase0=None,
                    momentum=0.0):
    """audio_lib.py:249-274.  stft_amp [1+n_fft//2, F] -> wav [hop*(F-1)].  The initial phase comes
    from the global numpy generator exactly like the reference (``np.random.seed`` makes both
    reproducible) unless ``phase0`` [bins, F] is given.  verbose prints the reference's
    per-iteration ``mrse_delta`` lines (after the run: the iterations are queued asynchronously).
    momentum: fast Griffin-Lim, see griffin_lim_batch."""
    momentum = check_momentum(momentum)
    stft_amp = np.asarray(stft_amp)
    if phase0 is None:
        phase0 = np.pi * np.random.rand(*stft_amp.shape)
    amp = np.ascontiguousarray(stft_amp.T, dtype=np.float32)[None]
    ph = np.ascontiguousarray(np.asarray(phase0).T, dtype=np.float32)[None]
    r = griffin_lim_batch(amp, None, win_length, hop_length, num_iters, n_fft, ph, trace=bool(verbose),
                          momentum=momentum)
    if verbose:
        wav, tr = r
        tr = tr.cpu().numpy()[:, 0]
        for i in range(1, int(num_iters)):
            print(' i={}  mrse_delta = {}'.format(i, np.sqrt(tr[i] / max(wav.shape[1], 1))))
    else:
        wav = r
    return wav[0].cpu().numpy()


def from_power_to_wav_batch(P, n_frames=None, P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=40,
                            win_length=800, mean_abs_amp_norm=0.01, n_iter=200, n_fft=None, realse=1.0,
                            phase0=None, trace=False, momentum=0.0, seed=0, utt_ids=None):
    """Batched from_power_to_wav: P [B, Fmax, bins] normalised power dB (the decoder's y_stft) ->
    wav [B, hop*(Fmax-1)] cuda float32; utterance b is valid up to hop*(n_frames[b]-1) samples.
    momentum: fast Griffin-Lim; phase0 / seed / utt_ids: see griffin_lim_batch."""
    import torch
    momentum = check_momentum(momentum)
    _check_phase0_name(phase0)
    if not torch.cuda.is_available():
        raise _vc.VCError('from_power_to_wav needs a GPU (no CPU fallback)')
    plan = _get_voc_plan(win_length, hop_length, n_fft)
    if not torch.is_tensor(P):
        P = torch.from_numpy(np.ascontiguousarray(P, dtype=np.float32))
    P = P.to(device='cuda', dtype=torch.float32).contiguous()
    if P.dim() != 3 or P.shape[2] != plan.n_bins:
        raise ValueError(' - ERROR, from_power_to_wav_batch: P must be [B, F, {}]'.format(plan.n_bins))
    B, Fmax, nb = P.shape
    d_nf, _ = _frames_arg(n_frames, B, Fmax, plan)
    amp = torch.empty_like(P)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(P), _vc.ptr(d_nf), B, Fmax, nb, float(P_dB_norm_factor), float(realse),
                                        _vc.ptr(amp), _vc.current_stream()))
    r = griffin_lim_batch(amp, n_frames, win_length, hop_length, n_iter, n_fft, phase0, trace, momentum, seed, utt_ids)
    wav = r[0] if trace else r
    _vc.check(_vc.lib().vc_inv_preemphasis_normalize(plan.handle, _vc.ptr(wav), _vc.ptr(d_nf), B, Fmax, wav.shape[1],
                                                     float(pre_emphasis), float(mean_abs_amp_norm), _vc.current_stream()))
    return r


def from_power_to_wav(P, P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=40, win_length=800,
                      mean_abs_amp_norm=0.01, n_iter=200, n_fft=None, realse=1.0, verbose=True, phase0=None,
                      momentum=0.0):
    """audio_lib.py:278-308.  P [F, bins] -> wav float32 numpy [hop*(F-1)].  momentum: fast
    Griffin-Lim, see griffin_lim_batch."""
    momentum = check_momentum(momentum)
    P = np.asarray(P)
    if phase0 is None:
        phase0 = np.pi * np.random.rand(P.shape[1], P.shape[0])          # [bins, F] like audio_lib.py:255
    ph = np.ascontiguousarray(np.asarray(phase0).T, dtype=np.float32)[None]
    r = from_power_to_wav_batch(np.ascontiguousarray(P, dtype=np.float32)[None], None, P_dB_norm_factor, pre_emphasis,
                                hop_length, win_length, mean_abs_amp_norm, n_iter, n_fft, realse, ph, trace=bool(verbose),
                                momentum=momentum)
    if verbose:
        wav, tr = r
        tr = tr.cpu().numpy()[:, 0]
        for i in range(1, int(n_iter)):
            print(' i={}  mrse_delta = {}'.format(i, np.sqrt(tr[i] / max(wav.shape[1], 1))))
    else:
        wav = r
    return wav[0].cpu().numpy()


# --------------------------------------------------------------------------- resampling
# res_type -> (zero crossings per side, roll-off, Kaiser beta): resampy's published presets.
RES_TYPES = {'kaiser_best': (64, 0.9475937167399596, 14.769656459379492),
             'kaiser_fast': (16, 0.85, 8.555504641634386)}
_RES_PLANS = {}


def _check_rate(sr, what):
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or int(sr) <= 0:
        raise ValueError(' - ERROR, resample: {} must be a positive integer rate, got {!r}'.format(what, sr))
    return int(sr)


def _res_params(res_type):
    if isinstance(res_type, str):
        if res_type not in RES_TYPES:
            raise ValueError(' - ERROR, resample: unknown res_type {!r} (known: {}, or a (Z, rolloff, beta) tuple)'
                             .format(res_type, ', '.join(sorted(RES_TYPES))))
        return RES_TYPES[res_type]
    try:
        z, rolloff, beta = res_type
        z, rolloff, beta = int(z), float(rolloff), float(beta)
    except (TypeError, ValueError):
        raise ValueError(' - ERROR, resample: unknown res_type {!r}'.format(res_type)) from None
    if z <= 0 or not 0.0 < rolloff <= 1.0 or not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError(' - ERROR, resample: res_type (Z, rolloff, beta) needs Z > 0, 0 < rolloff <= 1, beta >= 0, got {!r}'
                         .format(res_type))
    return z, rolloff, beta


def _ratio(sr_in, sr_out):
    sr_in, sr_out = _check_rate(sr_in, 'sr_in'), _check_rate(sr_out, 'sr_out')
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def resample_taps(sr_in, sr_out, res_type='kaiser_best'):
    """(up, down, half, taps): the Kaiser-windowed sinc of include/vc_hip.h ("Resampling") sampled in the up-sampled
    domain, taps[k + half] = h(k / up) for |k| <= half = ceil(Z * up / fc) - 1, float64.  Host only."""
    from scipy import special
    up, down = _ratio(sr_in, sr_out)
    z, rolloff, beta = _res_params(res_type)
    fc = rolloff * min(1.0, up / down)
    half = int(math.ceil(z * up / fc)) - 1
    t = np.arange(-half, half + 1, dtype=np.float64) / up
    w = 1.0 - (t * fc / z) ** 2
    inside = w > 0.0
    taps = np.where(inside, fc * np.sinc(fc * t) * special.i0(beta * np.sqrt(np.where(inside, w, 0.0))) / special.i0(beta), 0.0)
    return up, down, half, taps


def resample_len(n, sr_in, sr_out):
    """ceil(n * sr_out / sr_in) in exact integers (librosa.load's length); n an int or an integer array."""
    up, down = _ratio(sr_in, sr_out)
    if isinstance(n, (int, np.integer)):
        return (int(n) * up + down - 1) // down
    return (np.asarray(n, dtype=np.int64) * up + down - 1) // down


class _ResPlan:
    def __init__(self, sr_in, sr_out, res_type):
        self.up, self.down, self.half, taps = resample_taps(sr_in, sr_out, res_type)
        self._taps = np.ascontiguousarray(taps, dtype=np.float64)
        h = C.c_void_p()
        _vc.check(_vc.lib().vc_resample_plan_create(self.up, self.down, self.half, _vc.ptr(self._taps), C.byref(h)))
        self.handle = h


def _get_res_plan(sr_in, sr_out, res_type):
    up, down = _ratio(sr_in, sr_out)
    key = (up, down, res_type if isinstance(res_type, str) else tuple(res_type))
    p = _RES_PLANS.get(key)
    if p is None:
        p = _RES_PLANS[key] = _ResPlan(down, up, res_type)      # the taps depend on the ratio alone: rates down -> up
    return p


def _resample_launch(plan, wav, d_lens, out=None):
    """The one launch of resample_batch on validated device tensors (wav float32 [B, L] with unit sample stride, d_lens
    int32 [B] or None): no host check, copy or wait in here."""
    import torch
    B, L = wav.shape
    Lout = (L * plan.up + plan.down - 1) // plan.down
    if out is None:
        out = torch.empty((B, Lout), dtype=torch.float32, device=wav.device)
    # (the stride of a one-row tensor is arbitrary)
    _vc.check(_vc.lib().vc_resample_f32(plan.handle, _vc.ptr(wav), _vc.ptr(d_lens), B, L, wav.stride(0) if B > 1 else L,
                                        _vc.ptr(out), Lout, out.stride(0) if B > 1 else Lout, _vc.current_stream()))
    return out


def resample_batch(wav, lens=None, sr_in=None, sr_out=16000, res_type='kaiser_best', out=None):
    """Sample-rate conversion of a ragged batch on the GPU (vc_resample_f32, include/vc_hip.h): what
    librosa.load(path, sr_out) does to a file recorded at sr_in.

    wav  : float32 [B, Lmax] torch.cuda tensor (rows may be strided, samples contiguous) or numpy array (uploaded).
    lens : optional per-utterance sample counts at sr_in (host ints); None = all Lmax.
    res_type : 'kaiser_best', 'kaiser_fast' or a (Z, rolloff, beta) tuple.
    out  : optional preallocated float32 cuda tensor [B, resample_len(Lmax, sr_in, sr_out)].
    Returns (wav_out cuda float32 [B, resample_len(Lmax)], lens_out host int64 array); rows are zero from their own
    lens_out on.  sr_in == sr_out is the identity: nothing is launched and ``wav`` itself comes back."""
    import torch
    if sr_in is None:
        raise ValueError(' - ERROR, resample_batch: sr_in (the rate of wav) is required')
    up, down = _ratio(sr_in, sr_out)
    _res_params(res_type)
    if getattr(wav, 'ndim', 0) != 2:
        raise ValueError(' - ERROR, resample_batch: wav must be [B, Lmax]')
    B, L = int(wav.shape[0]), int(wav.shape[1])
    if B <= 0 or L <= 0:
        raise ValueError(' - ERROR, resample_batch: wav must be [B, Lmax] with B > 0 and Lmax > 0')
    h_lens = np.full((B,), L, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    if h_lens.shape != (B,) or h_lens.min() <= 0 or h_lens.max() > L:
        raise ValueError(' - ERROR, resample_batch: lens must be [B] with 0 < len <= Lmax')
    if up == down:
        return wav, h_lens
    Lout = (L * up + down - 1) // down
    if Lout >= 2 ** 31:
        raise ValueError(' - ERROR, resample_batch: {} output samples per row exceed int32'.format(Lout))
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != (B, Lout) or out.dtype != torch.float32
                            or not out.is_cuda or out.stride(1) != 1):
        raise ValueError(' - ERROR, resample_batch: out must be a float32 cuda tensor [{}, {}]'.format(B, Lout))
    if not torch.cuda.is_available():
        raise _vc.VCError('resample_batch needs a GPU (no CPU fallback)')
    plan = _get_res_plan(sr_in, sr_out, res_type)
    if not torch.is_tensor(wav):
        wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    wav = wav.to(device='cuda', dtype=torch.float32)
    if wav.stride(1) != 1 or (B > 1 and wav.stride(0) < L):
        wav = wav.contiguous()
    d_lens = None
    if lens is not None:
        d_lens = torch.from_numpy(h_lens.astype(np.int32)).pin_memory().to('cuda', non_blocking=True)
    return _resample_launch(plan, wav, d_lens, out), (h_lens * up + down - 1) // down


def resample(y, orig_sr, target_sr, res_type='kaiser_best'):
    """One utterance, numpy in, numpy float32 out [ceil(len * target_sr / orig_sr)]: the resampling half of
    librosa.load(path, target_sr).  Equal rates return ``y`` itself."""
    up, down = _ratio(orig_sr, target_sr)
    _res_params(res_type)
    if up == down:
        return y
    y = np.ascontiguousarray(np.asarray(y).reshape(1, -1), dtype=np.float32)
    out, _ = resample_batch(y, None, orig_sr, target_sr, res_type)
    return out[0].cpu().numpy()
