"""Timing of the noise suppression (csrc/vc_denoise.hip and the power kernels of csrc/vc_vocoder.hip behind
audio_lib.stft_power_batch, enhance.noise_gain_batch / denoise_batch and denoise= of the conversion entry points) on one
MI355X: HIP events, arms interleaved, medians.

Kernels, 16 utterances x 5 s at 16 kHz (1,001 frames x 201 bins, hop 80), synthetic speech with white noise at 10 dB:
  a float4 copy of the power slab (torch's copy_); vc_stft_power_f32; vc_noise_gain_f32 with both rules, with and without
  the noise track; vc_stft_filter_f32 (its two launches); and the whole denoise_batch chain.  Event figures include the
  launch gap of a call from Python and the allocations of the outputs.
Calls, the same audio, bf16 models:
  convert_batch (32 iterations of fast Griffin-Lim) and convert_diff_batch, each without and with denoise=True.

    python tools/ab_denoise.py --reps 7 --out profiles/denoise/ab_denoise.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_pitch import B, F, HOP, L                                   # noqa: E402  (the same sizes)
from ab_warp import interleaved                                     # noqa: E402  (the same timing loops)

SR, N_FFT = 16000, 400
NB = 1 + N_FFT // 2


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
    import enhance
    if not torch.cuda.is_available():
        raise SystemExit('ab_denoise needs a GPU')
    from bench import synth_audio
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t):
        med = {}
        for k, v in t.items():
            med[k] = float(np.median(v))
            say('  %-60s median %9.4f ms  (min %.4f, max %.4f, %d reps)' % (k, med[k], min(v), max(v), len(v)))
        return med

    def finish():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    # ---- kernels
    clean = synth_audio(B, L, seed=300)
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(clean.shape, generator=g) * float(clean.pow(2).mean().sqrt()) * 10.0 ** (-10.0 / 20.0)
    wav = (clean + noise).cuda()
    d_len = torch.full((B,), L, dtype=torch.int32, device='cuda')
    plan = audio_lib._get_voc_plan(N_FFT, HOP, N_FFT)
    cfg = {rule: enhance.gain_cfg('ab_denoise', rule=rule, hop_length=HOP, sr=SR) for rule in enhance.RULES}
    power, d_nf = audio_lib._stft_power_launch(plan, wav, d_len, None, F)
    gain, _ = enhance._noise_gain_launch(power, d_nf, None, cfg['logmmse'], False)
    dst = torch.empty_like(power)
    att = 10.0 * torch.log10(power.sum() / (gain * gain * power).sum())
    say('input: %d x %d samples, white noise 10 dB under the synthetic speech; the gain takes %.2f dB off the total power'
        % (B, L, float(att)))
    arms = {'float4 copy of the power slab (torch copy_)': lambda: dst.copy_(power),
            'vc_stft_power_f32': lambda: audio_lib._stft_power_launch(plan, wav, d_len, None, F),
            'vc_noise_gain_f32, log-MMSE': lambda: enhance._noise_gain_launch(power, d_nf, None, cfg['logmmse'], False),
            'vc_noise_gain_f32, log-MMSE, with the noise track': lambda: enhance._noise_gain_launch(power, d_nf, None, cfg['logmmse'], True),
            'vc_noise_gain_f32, Wiener': lambda: enhance._noise_gain_launch(power, d_nf, None, cfg['wiener'], False),
            'vc_stft_filter_f32 (filter and overlap-add)': lambda: audio_lib._stft_filter_launch(plan, wav, d_len, gain, d_nf),
            'denoise_batch, every launch': lambda: enhance._denoise_launch(plan, wav, d_len, None, F, cfg['logmmse'], None, False)}
    say('kernels at %d x %d frames x %d bins (HIP events over %d back-to-back calls, launch gaps and allocations included)'
        % (B, F, NB, a.inner))
    report(interleaved(arms, a.reps, a.inner))
    if a.kernels_only:
        return finish()

    # ---- the calls
    from ab_convert_batch import models
    dec, c = models()
    lens = [L] * B
    kw = dict(n_iter=32, momentum=0.99, phase='device', seed=1)
    calls = {'convert_batch (32 iterations, momentum 0.99)': lambda: conversion.convert_batch(dec, wav, lens, c, **kw),
             'convert_batch(denoise=True)': lambda: conversion.convert_batch(dec, wav, lens, c, denoise=True, **kw),
             'convert_diff_batch': lambda: conversion.convert_diff_batch(dec, wav, lens, c),
             'convert_diff_batch(denoise=True)': lambda: conversion.convert_diff_batch(dec, wav, lens, c, denoise=True)}
    say('calls on 16 x 5 s, bf16 models (HIP events around one call)')
    for f in calls.values():
        f()
    med = report(interleaved(calls, a.reps, 1))
    k = list(calls)
    say('  denoise=True adds %.3f ms to convert_batch and %.3f ms to convert_diff_batch'
        % (med[k[1]] - med[k[0]], med[k[3]] - med[k[2]]))
    finish()


if __name__ == '__main__':
    main()
