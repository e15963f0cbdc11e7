"""Timing of waveform time scaling (csrc/vc_wsola.hip behind conversion.time_scale_batch / convert_diff_duration_batch) on one
MI355X: HIP events, arms interleaved, medians, with the spread.

Kernels, 16 utterances x 80,000 samples (16 x 5 s at 16 kHz), hop 80, group 2, tol 160 (the defaults), speech-like audio:
  vc_wsola_plan and vc_wsola_ola_f32 at rate 1.25 (1,251 output frames, 626 grains) and at rate 0.5 (500 frames, 251
  grains), each alone; vc_wsola_ola_f32 against a float4 copy of the bytes it moves (every output sample reads two input
  samples and is written once).  Event figures include the launch gap of a call from Python.
Calls, 16 x 5 s of synthetic audio, bf16 models:
  convert_diff_duration_batch(rate=1.0) against convert_diff_batch (the cost of the feature) and against
  convert_duration_batch(rate=1.0) with 32 iterations at momentum 0.99.

    python tools/ab_wsola.py --reps 7 --out profiles/wsola/ab_wsola.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_warp import interleaved                                     # noqa: E402  (the same timing loops)

B, L, HOP, GROUP, TOL = 16, 80000, 80, 2, 160
F = 1 + L // HOP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10, help='back-to-back launches per kernel timing')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import conversion
    from bench import synth_audio
    if not torch.cuda.is_available():
        raise SystemExit('ab_wsola needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t, notes=None):
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, v in t.items():
            say('  %-62s median %9.4f ms  (min %.4f, max %.4f, spread %.1f %%, %d reps)%s'
                % (k, med[k], min(v), max(v), 100 * (max(v) - min(v)) / med[k], len(v), (notes or {}).get(k, '')))
        return med

    def finish():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    # ---- kernels
    wav = synth_audio(B, L, seed=300).cuda().contiguous()
    wav = wav * (0.5 / wav.abs().max())
    d_len = torch.full((B,), L, dtype=torch.int32, device='cuda')
    one = np.ones((B,), np.int32)
    arms, notes = {}, {}
    for rate in (1.25, 0.5):
        m = conversion.duration_map_batch(np.zeros((B, 1), np.int32), np.full((B, 1), F, np.int32), one, np.full((B,), F), ratio=rate)
        p = conversion._wsola_plan_launch(wav, d_len, m.pos, m.n_out, HOP, GROUP, TOL, 32768.0)
        y = conversion._wsola_ola_launch(wav, d_len, p)
        torch.cuda.synchronize()
        K, n_out, cost = int(p.n_grains[0]), int(m.n_out[0]), p.cost[:, 1:int(p.n_grains[0])].double()
        moved = (p.a[:, :K] - p.a[:, :K].clone().roll(1, 1))[:, 1:] != GROUP * HOP
        say('rate %.2f: %d output frames, %d grains per utterance; mean cost per sample of a grain %.1f of 32768; %.0f %% of the grains '
            'are not the continuation of their predecessor' % (rate, n_out, K, float(cost.mean()) / (2 * GROUP * HOP), 100 * float(moved.double().mean())))
        nb = 4 * B * int(p.out_len[0]) * 3
        src, dst = torch.empty(nb // 8, device='cuda'), torch.empty(nb // 8, device='cuda')
        k1, k2, k3 = ('vc_wsola_plan, rate %.2f (%d dependent steps)' % (rate, K - 1), 'vc_wsola_ola_f32, rate %.2f' % rate,
                      'float4 copy of the overlap-add\'s %.1f MB, rate %.2f' % (nb / 1e6, rate))
        arms[k1] = (lambda m=m: conversion._wsola_plan_launch(wav, d_len, m.pos, m.n_out, HOP, GROUP, TOL, 32768.0))
        arms[k2] = (lambda p=p: conversion._wsola_ola_launch(wav, d_len, p))
        arms[k3] = (lambda src=src, dst=dst: dst.copy_(src))
        notes[k1] = '  per step: see below'
        del y
    say('kernels at %d x %d samples, hop %d, group %d, tol %d (HIP events over %d back-to-back calls, launch gaps and the calls\' allocations '
        'included)' % (B, L, HOP, GROUP, TOL, a.inner))
    med = report(interleaved(arms, a.reps, a.inner))
    for k, v in med.items():
        if k.startswith('vc_wsola_plan'):
            steps = int(k.split('(')[1].split()[0])
            say('  %s: %.2f us per dependent step' % (k, 1e3 * v / steps))
    if a.kernels_only:
        return finish()

    # ---- the calls
    from ab_convert_batch import models
    dec, c = models()
    lens = [L] * B
    wav = synth_audio(B, L, seed=300).cuda()
    calls = {'convert_diff_batch': lambda: conversion.convert_diff_batch(dec, wav, lens, c),
             'convert_diff_duration_batch, rate 1.0': lambda: conversion.convert_diff_duration_batch(dec, wav, lens, c, rate=1.0),
             'convert_diff_duration_batch, rate 1.25': lambda: conversion.convert_diff_duration_batch(dec, wav, lens, c, rate=1.25),
             'convert_duration_batch, rate 1.0, 32 iterations at momentum 0.99': lambda: conversion.convert_duration_batch(
                 dec, wav, lens, c, rate=1.0, n_iter=32, momentum=0.99, seed=1)}
    r0, r1, r2, _ = (f() for f in calls.values())
    n = r0.n_samples[0]
    assert torch.equal(r1.y_wav_pred[:, :n], r0.y_wav_pred[:, :n]) and torch.isfinite(r2.y_wav_pred).all()
    say('calls on 16 x 5 s, bf16 models (HIP events around one call); rate 1.0 returns convert_diff_batch\'s waveform bit for bit; frames per '
        'utterance: %d, at rate 1.25: %d' % (r0.n_frames[0], int(r2.n_frames[0])))
    med = report(interleaved(calls, a.reps, 1))
    d = med['convert_diff_duration_batch, rate 1.0'] - med['convert_diff_batch']
    say('  the feature costs %.3f ms at rate 1.0: %.1f %% on top of convert_diff_batch; convert_diff_duration_batch takes %.1f %% of '
        'convert_duration_batch' % (d, 100 * d / med['convert_diff_batch'], 100 * med['convert_diff_duration_batch, rate 1.0']
                                    / med['convert_duration_batch, rate 1.0, 32 iterations at momentum 0.99']))
    finish()


if __name__ == '__main__':
    main()
