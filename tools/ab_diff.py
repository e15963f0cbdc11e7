"""Timing of differential-spectrum conversion (the two launches added to csrc/vc_vocoder.hip behind
conversion.diff_gain_batch / audio_lib.stft_filter_batch / conversion.convert_diff_batch) on one MI355X: HIP events, arms
interleaved, medians, with the spread.

Kernels, 16 utterances x 80,000 samples (16 x 5 s at 16 kHz), 1,001 frames of 201 bins:
  vc_spectral_diff_gain_f32 (17 taps) against a float4 copy of the bytes it moves (two spectra read, one gain written);
  vc_stft_filter_f32 (the filter kernel and the overlap-add kernel) against a float4 copy of its bytes (the gain and the
  waveform read, the frames written and read again, the waveform written); one plain Griffin-Lim iteration on the same
  shape next to it (vc_griffin_lim_f32 at 2 iterations minus 1 iteration).  Event figures include the launch gap of a call
  from Python.
Calls, 16 x 5 s of synthetic audio, bf16 models:
  convert_diff_batch; convert_batch with 32 iterations at momentum 0.99; convert_batch with 200 plain iterations.

    python tools/ab_diff.py --reps 7 --out profiles/diff/ab_diff.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_warp import interleaved                                     # noqa: E402  (the same timing loops)

B, L, HOP, NB, N = 16, 80000, 80, 201, 400
F = 1 + L // HOP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50, help='back-to-back launches per kernel timing')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import audio_lib
    import conversion
    if not torch.cuda.is_available():
        raise SystemExit('ab_diff needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t, nbytes=None, copies=None):
        med = {}
        for k, v in t.items():
            med[k] = float(np.median(v))
        for k, v in t.items():
            extra = ''
            if nbytes and k in nbytes:
                extra = '  %.1f MB, %.2f TB/s' % (nbytes[k] / 1e6, nbytes[k] / (med[k] * 1e-3) / 1e12)
                if copies and k in copies:
                    extra += ', %.2f x its copy' % (med[k] / med[copies[k]])
            say('  %-58s median %9.4f ms  (min %.4f, max %.4f, spread %.1f %%, %d reps)%s'
                % (k, med[k], min(v), max(v), 100 * (max(v) - min(v)) / med[k], len(v), extra))
        return med

    # ---- kernels
    g = torch.Generator().manual_seed(1)
    pred, tru = (torch.rand((B, F, NB), generator=g).cuda() for _ in range(2))
    x = (torch.rand((B, L), generator=g) - 0.5).cuda()
    d_len = torch.full((B,), L, dtype=torch.int32, device='cuda')
    d_nf = torch.full((B,), F, dtype=torch.int32, device='cuda')
    d_taps = torch.from_numpy(conversion.diff_smoothing_taps(8)).cuda()
    plan = audio_lib._get_voc_plan(N, HOP, N)
    gain = conversion._diff_gain_launch(pred, tru, d_nf, 0.01, 1.0, 20.0, 30.0, d_taps)
    amp, ph = torch.rand((B, F, NB), generator=g).cuda(), (3.14 * torch.rand((B, F, NB), generator=g)).cuda()
    spec, frames = 4 * B * F * NB, 4 * B * F * N
    wave = 4 * B * HOP * (F - 1)
    b_gain, b_filter = 3 * spec, spec + 4 * B * L + 2 * frames + wave
    src_g, dst_g = torch.empty(b_gain // 8, device='cuda'), torch.empty(b_gain // 8, device='cuda')
    src_f, dst_f = torch.empty(b_filter // 8, device='cuda'), torch.empty(b_filter // 8, device='cuda')
    arms = {'float4 copy of the gain launch\'s bytes': lambda: dst_g.copy_(src_g),
            'vc_spectral_diff_gain_f32, 17 taps': lambda: conversion._diff_gain_launch(pred, tru, d_nf, 0.01, 1.0, 20.0, 30.0, d_taps),
            'float4 copy of the filter call\'s bytes': lambda: dst_f.copy_(src_f),
            'vc_stft_filter_f32 (filter + overlap-add)': lambda: audio_lib._stft_filter_launch(plan, x, d_len, gain, d_nf),
            'vc_griffin_lim_f32, 1 iteration (initial + overlap-add)': lambda: audio_lib._griffin_lim_launch(plan, amp, ph, d_nf, 1, False, 0.0),
            'vc_griffin_lim_f32, 2 iterations': lambda: audio_lib._griffin_lim_launch(plan, amp, ph, d_nf, 2, False, 0.0)}
    nbytes = {'float4 copy of the gain launch\'s bytes': b_gain, 'vc_spectral_diff_gain_f32, 17 taps': b_gain,
              'float4 copy of the filter call\'s bytes': b_filter, 'vc_stft_filter_f32 (filter + overlap-add)': b_filter}
    copies = {'vc_spectral_diff_gain_f32, 17 taps': 'float4 copy of the gain launch\'s bytes',
              'vc_stft_filter_f32 (filter + overlap-add)': 'float4 copy of the filter call\'s bytes'}
    say('kernels at %d x %d samples, %d frames (HIP events over %d back-to-back calls, launch gaps and the calls\' allocations included)'
        % (B, L, F, a.inner))
    med = report(interleaved(arms, a.reps, a.inner), nbytes, copies)
    say('  one plain Griffin-Lim iteration on this shape (2 iterations minus 1): %.4f ms'
        % (med['vc_griffin_lim_f32, 2 iterations'] - med['vc_griffin_lim_f32, 1 iteration (initial + overlap-add)']))

    def finish():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    if a.kernels_only:
        return finish()

    # ---- the calls
    from ab_convert_batch import models
    from bench import synth_audio
    dec, c = models()
    lens = [L] * B
    wav = synth_audio(B, L, seed=300).cuda()
    calls = {'convert_diff_batch': lambda: conversion.convert_diff_batch(dec, wav, lens, c),
             'convert_batch, 32 iterations at momentum 0.99': lambda: conversion.convert_batch(dec, wav, lens, c, n_iter=32, momentum=0.99,
                                                                                               phase='device', seed=1),
             'convert_batch, 200 plain iterations': lambda: conversion.convert_batch(dec, wav, lens, c, n_iter=200, phase='device', seed=1)}
    r0, r1, _ = (f() for f in calls.values())
    assert torch.equal(r0.stft_pred, r1.stft_pred) and torch.isfinite(r0.y_wav_pred).all()
    say('calls on 16 x 5 s, bf16 models (HIP events around one call); the three share their spectra bit for bit; frames filtered per '
        'utterance: %d of %d converted' % (r0.n_frames[0], r1.n_frames[0]))
    med = report(interleaved(calls, a.reps, 1))
    say('  convert_diff_batch takes %.3f ms: %.1f %% of the 32-iteration call, %.1f %% of the 200-iteration call'
        % (med['convert_diff_batch'], 100 * med['convert_diff_batch'] / med['convert_batch, 32 iterations at momentum 0.99'],
           100 * med['convert_diff_batch'] / med['convert_batch, 200 plain iterations']))
    finish()


if __name__ == '__main__':
    main()
