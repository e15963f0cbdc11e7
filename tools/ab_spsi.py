"""The deterministic phase start (vc_phase_spsi, phase0='spsi') against the random one (vc_phase_init, phase0='device') on one
box, in one process, interleaved (ABAB...), at the bench's vocoder shape (16 utterances x 1000 frames, n_fft 400, hop 80,
bench.py's synthetic audio):

  1. us per call of phase_spsi (its three launches together) and of phase_init, and us per plain and per momentum
     iteration of the iteration kernel from the same run (HIP events; (t200 - t20) / 180 as tools/ab_fgla.py) -- the cost
     of the start in iterations.  HIP events cannot separate launches that one ABI call enqueues: the three kernels' own
     times come from `rocprofv3 --kernel-trace --stats -- python tools/ab_spsi.py --kernels`, a run of its own;
  2. the spectral convergence || |STFT(y)| - A || / ||A|| the device reaches from either start at momentum 0.99 with
     num_iters in 1, 5, 9, 17, 33, 51 and at momentum 0 with 200 (mean over the 16 utterances, float64 evaluation on the
     host), for the front-end's power spectra (consistent) and for the same spectra with 2 dB of seeded noise per bin
     (inconsistent, a stand-in for decoder predictions: the repository carries no trained decoder);
  3. per kind of spectra, the smallest num_iters from the SPSI start whose SC is no worse than ('device', 0.99, 33)
     (bisection between the counts of the table) and from_power_to_wav_batch frames/s there, next to that setting's own
     on the same spectra.
The event loops of step 1 call each function back to back on the same 12.9 MB of magnitudes, which stay warm in L2 and
the Infinity Cache; the kernel trace interleaves Griffin-Lim iterations that evict them, so its durations are the colder
figure.
Prints one JSON line per measurement and a summary line.
python tools/ab_spsi.py [--reps 5] [--steps 5] [--kernels]"""
import argparse
import json
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
ALPHA = 0.99
ITERS = (1, 5, 9, 17, 33, 51)
TARGET = 33
STARTS = ('device', 'spsi')


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


def mean_sc(A, A_h, start, m, n):
    y = audio_lib.griffin_lim_batch(A, None, 400, 80, n, None, start, momentum=m, seed=300).cpu().numpy()
    return float(np.mean([vo.spectral_convergence(y[b], A_h[b].T, 400, 80) for b in range(B)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--kernels', action='store_true', help='only a short loop of the launches, for a kernel trace')
    a = ap.parse_args()
    wav = synth_audio(B, 80 * (F - 1), seed=300).cuda()
    _, _, P = audio_lib.calc_MFCC_input_batch(wav, None, **FE_KW)
    P = P[:, :F].contiguous()
    noise = torch.from_numpy(np.random.RandomState(5).standard_normal((B, F, 201)).astype(np.float32)).cuda()
    P_noisy = torch.clamp(P + 0.02 * noise, min=0.0)   # P is dB / 100: 0.02 = 2 dB
    amp = power_to_amp(P)
    ph = torch.empty_like(amp)
    nf = [F] * B

    if a.kernels:
        for _ in range(20):
            audio_lib.phase_spsi(amp, None, 80, 400, out=ph)
            audio_lib.phase_init(nf, F, 201, 300, None, out=ph)
            audio_lib.griffin_lim_batch(amp, None, 400, 80, 9, None, ph, momentum=ALPHA)
        torch.cuda.synchronize()
        return

    # 1. the start's cost and the iteration's, ABAB
    d_nf = torch.tensor(nf, dtype=torch.int32, device='cuda')
    calls = {'phase_spsi': lambda: audio_lib.phase_spsi(amp, None, 80, 400, out=ph),
             'phase_init': lambda: audio_lib.phase_init(d_nf, F, 201, 300, None, out=ph)}
    us = {k: [] for k in list(calls) + ['iteration_0', 'iteration_0.99']}
    for r in range(a.reps):
        for k, fn in calls.items():
            us[k].append(events(fn, 20 * a.steps) * 1e3)
        for m in (0.0, ALPHA):
            t = {n: events(lambda: audio_lib.griffin_lim_batch(amp, None, 400, 80, n, None, ph, momentum=m), a.steps)
                 for n in (200, 20)}
            us['iteration_%g' % m].append((t[200] - t[20]) * 1e3 / 180.0)
    med = {k: float(np.median(v)) for k, v in us.items()}
    cost = {'spsi_in_momentum_iterations': round(med['phase_spsi'] / med['iteration_0.99'], 2),
            'spsi_in_plain_iterations': round(med['phase_spsi'] / med['iteration_0'], 2),
            'phase_init_in_momentum_iterations': round(med['phase_init'] / med['iteration_0.99'], 2)}
    moved = 3 * B * F * 201 * 4 + _vc.lib().vc_phase_spsi_workspace_bytes(B, F, 201)
    print(json.dumps({'measure': 'us_per_call', 'shape': [B, F], 'samples': {k: [round(x, 2) for x in v] for k, v in us.items()},
                      'median': {k: round(v, 2) for k, v in med.items()}, **cost,
                      'spsi_bytes_amp_twice_phase_once_tables': moved,
                      'spsi_GB_per_s': round(moved / (med['phase_spsi'] * 1e-6) / 1e9, 1)}), flush=True)

    # 2. spectral convergence on the device
    sc_all, need = {}, {}
    for name, PP in (('consistent', P), ('noisy_2dB', P_noisy)):
        A = power_to_amp(PP)
        A_h = A.cpu().numpy().astype(np.float64)
        sc = {}
        for s in STARTS:
            for n in ITERS:
                sc['%s,%g,%d' % (s, ALPHA, n)] = mean_sc(A, A_h, s, ALPHA, n)
            sc['%s,0,200' % s] = mean_sc(A, A_h, s, 0.0, 200)
        sc_all[name] = {k: round(v, 5) for k, v in sc.items()}
        print(json.dumps({'measure': 'spectral_convergence', 'input': name, 'mean_over_utterances': sc_all[name]}), flush=True)
        # 3a. the smallest count from the SPSI start that is no worse than ('device', 0.99, 33)
        goal = sc['device,%g,%d' % (ALPHA, TARGET)]
        ok = [n for n in ITERS if sc['spsi,%g,%d' % (ALPHA, n)] <= goal]
        if not ok:
            need[name] = None
        else:
            hi = ok[0]
            lo = max([n for n in ITERS if n < hi], default=0)       # lo fails (or is 0), hi passes
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if mean_sc(A, A_h, 'spsi', ALPHA, mid) <= goal:
                    hi = mid
                else:
                    lo = mid
            need[name] = hi
        print(json.dumps({'measure': 'spsi_num_iters_at_equal_sc', 'input': name, 'goal_sc_device_0.99_33': round(goal, 5),
                          'num_iters': need[name]}), flush=True)

    # 3b. end-to-end vocoder throughput at equal SC, ABAB
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80, win_length=400, mean_abs_amp_norm=0.045,
              n_fft=None, realse=1.0, momentum=ALPHA, seed=300)
    runs = {}
    for name, PP in (('consistent', P), ('noisy_2dB', P_noisy)):
        runs['device,%d,%s' % (TARGET, name)] = ('device', TARGET, PP)
        if need[name] is not None:
            runs['spsi,%d,%s' % (need[name], name)] = ('spsi', need[name], PP)
    fps = {k: [] for k in runs}
    for r in range(a.reps):
        for k, (s, n, PP) in runs.items():
            ms = events(lambda: audio_lib.from_power_to_wav_batch(PP, None, n_iter=n, phase0=s, **kw), a.steps)
            fps[k].append(B * F / (ms * 1e-3))
    fmed = {k: float(np.median(v)) for k, v in fps.items()}
    ratio = {k: round(v / fmed['device,%d,%s' % (TARGET, k.rsplit(',', 1)[1])], 2) for k, v in fmed.items()}
    print(json.dumps({'measure': 'from_power_to_wav_batch_frames_per_s', 'median': {k: round(v, 1) for k, v in fmed.items()},
                      'speedup_vs_device_%d_same_spectra' % TARGET: ratio}), flush=True)
    print(json.dumps({'summary': {'us': {k: round(v, 2) for k, v in med.items()}, **cost, 'sc': sc_all,
                                  'spsi_num_iters_at_equal_sc': need,
                                  'frames_per_s': {k: round(v, 1) for k, v in fmed.items()},
                                  'device': torch.cuda.get_device_name(0)}}), flush=True)


if __name__ == '__main__':
    main()
