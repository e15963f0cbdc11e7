"""Fast Griffin-Lim (momentum) against the plain loop on one box, in one process, interleaved (ABAB...), at the
bench's vocoder shape (16 utterances x 1000 frames, n_fft 400, hop 80, bench.py's synthetic audio and phase):

  1. us per iteration of the iteration kernel at momentum 0 and 0.99: HIP events around griffin_lim_batch with
     200 and with 20 iterations, (t200 - t20) / 180 (the initial spectrum and the final overlap-add cancel);
  2. frames/s of from_power_to_wav_batch at (0, 200), (0.99, 32), (0.99, 50);
  3. the spectral convergence || |STFT(y)| - A || / ||A|| each setting reaches on the device (mean over the 16
     utterances, float64 evaluation on the host), for the front-end's power spectra (consistent) and for the same
     spectra with 2 dB of seeded noise per bin (inconsistent, a stand-in for decoder predictions: the repository
     carries no trained decoder).
Prints one JSON line per measurement and a summary line.
python tools/ab_fgla.py [--reps 5] [--steps 5]"""
import argparse
import json
import math
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd')):
    sys.path.insert(0, p)
import numpy as np
import torch
import _vc
import audio_lib
from bench import FE_KW, synth_audio
from oracle import vocoder_oracle as vo

B, F = 16, 1000
SETTINGS = ((0.0, 200), (0.99, 32), (0.99, 50))


def events(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                     # ms per call


def power_to_amp(P):
    amp = torch.empty_like(P)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(P), None, B, F, 201, 0.01, 1.0, _vc.ptr(amp), _vc.current_stream()))
    return amp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(300)
    wav = synth_audio(B, 80 * (F - 1), seed=300).cuda()
    _, _, P = audio_lib.calc_MFCC_input_batch(wav, None, **FE_KW)
    P = P[:, :F].contiguous()
    ph = (torch.rand(B, F, 201, generator=g) * math.pi).cuda()
    noise = torch.from_numpy(np.random.RandomState(5).standard_normal((B, F, 201)).astype(np.float32)).cuda()
    P_noisy = torch.clamp(P + 0.02 * noise, min=0.0)   # P is dB / 100: 0.02 = 2 dB
    amp = power_to_amp(P)

    # 1. per-iteration cost, ABAB
    per_iter = {0.0: [], 0.99: []}
    for r in range(a.reps):
        for m in (0.0, 0.99):
            t = {n: events(lambda: audio_lib.griffin_lim_batch(amp, None, 400, 80, n, None, ph, momentum=m), a.steps)
                 for n in (200, 20)}
            per_iter[m].append((t[200] - t[20]) * 1e3 / 180.0)
    med = {m: float(np.median(v)) for m, v in per_iter.items()}
    print(json.dumps({'measure': 'us_per_iteration', 'shape': [B, F], 'samples': {str(k): [round(x, 2) for x in v]
                      for k, v in per_iter.items()}, 'median': {str(k): round(v, 2) for k, v in med.items()},
                      'ratio': round(med[0.99] / med[0.0], 3)}), flush=True)

    # 2. end-to-end vocoder throughput, ABAB over the three settings
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80, win_length=400, mean_abs_amp_norm=0.045,
              n_fft=None, realse=1.0, phase0=ph)
    fps = {s: [] for s in SETTINGS}
    for r in range(a.reps):
        for m, n in SETTINGS:
            ms = events(lambda: audio_lib.from_power_to_wav_batch(P, None, n_iter=n, momentum=m, **kw), a.steps)
            fps[(m, n)].append(B * F / (ms * 1e-3))
    fmed = {s: float(np.median(v)) for s, v in fps.items()}
    print(json.dumps({'measure': 'from_power_to_wav_batch_frames_per_s',
                      'median': {'%g,%d' % s: round(v, 1) for s, v in fmed.items()},
                      'speedup_vs_0_200': {'%g,%d' % s: round(v / fmed[(0.0, 200)], 2) for s, v in fmed.items()}}),
          flush=True)

    # 3. spectral convergence on the device
    sc_all = {}
    for name, PP in (('consistent', P), ('noisy_2dB', P_noisy)):
        A = power_to_amp(PP)
        A_h = A.cpu().numpy().astype(np.float64)
        sc = {}
        for m, n in SETTINGS:
            y = audio_lib.griffin_lim_batch(A, None, 400, 80, n, None, ph, momentum=m).cpu().numpy()
            sc['%g,%d' % (m, n)] = round(float(np.mean([vo.spectral_convergence(y[b], A_h[b].T, 400, 80)
                                                        for b in range(B)])), 5)
        sc_all[name] = sc
        print(json.dumps({'measure': 'spectral_convergence', 'input': name, 'mean_over_utterances': sc}), flush=True)
    print(json.dumps({'summary': {'us_per_iteration': {str(k): round(v, 2) for k, v in med.items()},
                                  'per_iteration_ratio': round(med[0.99] / med[0.0], 3),
                                  'frames_per_s': {'%g,%d' % s: round(v, 1) for s, v in fmed.items()},
                                  'sc': sc_all,
                                  'device': torch.cuda.get_device_name(0)}}), flush=True)


if __name__ == '__main__':
    main()
