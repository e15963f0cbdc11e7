"""Timing of the dereverberation (csrc/vc_dereverb.hip and the complex transform kernels of csrc/vc_vocoder.hip behind
audio_lib.stft_complex_batch / istft_complex_batch, enhance.wpe_batch / dereverb_batch and dereverb= of the conversion
entry points) on one MI355X: HIP events, arms interleaved, medians.

Kernels, 16 utterances x 5 s at 16 kHz (1,001 frames x 201 bins, hop 80), synthetic speech:
  vc_stft_complex_f32; vc_wpe_f32 at K in (8, 16, 32) and I in (1, 3), delay 5, context 1; vc_istft_complex_f32 (its two
  launches); the whole dereverb_batch chain; denoise_batch on the same input for scale.  Event figures include the launch
  gap of a call from Python and the allocations of the outputs.  Next to every solver time: its float64 operation count and
  the bytes it moves (the model is in solver_work below).
Calls, the same audio, bf16 models:
  convert_diff_batch without and with dereverb=True.

    python tools/ab_dereverb.py --reps 7 --out profiles/dereverb/ab_dereverb.log
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

SR, N_FFT, DELAY = 16000, 400, 5
NB = 1 + N_FFT // 2


def solver_work(K, I, frames=F, bins=NB, batch=B, delay=DELAY):
    """(float64 operations, bytes of global memory) of one vc_wpe_f32 launch.  Per bin and iteration: every entry of the
    upper triangle of R and of q is a sum over about F - D - j frames of one complex product (4 products, 2 sums), 2
    divisions and 2 additions: 10 operations a term (a division counted as one); y is K complex products and sums a frame
    (8 K); lam and |y|^2 a handful; the factorisation K^3 / 3 complex products (8 operations each) and the substitutions
    2 K^2.  Bytes: the two input planes read once, the two output planes written once, float32."""
    terms = sum(max(frames - delay - j, 0) for i in range(K) for j in range(i, K)) + sum(max(frames - delay - i, 0) for i in range(K))
    per_bin = I * (10 * terms + 8 * K * frames + 8 * frames + 8 * K ** 3 // 3 + 16 * K * K)
    return batch * bins * per_bin, 4 * 4 * batch * bins * frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10, help='back-to-back launches per kernel timing')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import audio_lib
    import conversion
    import enhance
    if not torch.cuda.is_available():
        raise SystemExit('ab_dereverb needs a GPU')
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
    wav = synth_audio(B, L, seed=300).cuda()
    d_len = torch.full((B,), L, dtype=torch.int32, device='cuda')
    plan = audio_lib._get_voc_plan(N_FFT, HOP, N_FFT)
    re, im, d_nf = audio_lib._stft_complex_launch(plan, wav, d_len, None, F)
    cfgs = {(K, I): enhance.wpe_cfg('ab_dereverb', taps=K, delay=DELAY, iterations=I) for K in (8, 16, 32) for I in (1, 3)}
    r = enhance._wpe_launch(re, im, d_nf, cfgs[(16, 3)], False)
    dcfg = enhance.gain_cfg('ab_dereverb', hop_length=HOP, sr=SR)
    say('input: %d x %d samples of synthetic speech; at K = 16, I = 3 every status is 0: %s' % (B, L, not bool(r.status.any())))
    arms = {'vc_stft_complex_f32': lambda: audio_lib._stft_complex_launch(plan, wav, d_len, None, F)}
    for (K, I), c in cfgs.items():
        arms['vc_wpe_f32, K = %d, I = %d' % (K, I)] = (lambda c=c: enhance._wpe_launch(re, im, d_nf, c, False))
    arms['vc_istft_complex_f32 (inverse and overlap-add)'] = lambda: audio_lib._istft_complex_launch(plan, r.re, r.im, d_nf)
    arms['dereverb_batch, every launch (K = 16, I = 3)'] = lambda: enhance._dereverb_launch(plan, wav, d_len, None, F, cfgs[(16, 3)], False)
    arms['denoise_batch, every launch'] = lambda: enhance._denoise_launch(plan, wav, d_len, None, F, dcfg, None, False)
    say('kernels at %d x %d frames x %d bins (HIP events over %d back-to-back calls, launch gaps and allocations included)'
        % (B, F, NB, a.inner))
    med = report(interleaved(arms, a.reps, a.inner))
    say('the solver against its own work (float64 operations counted as in solver_work; bytes: both planes in, both out)')
    for (K, I) in cfgs:
        ops, nbytes = solver_work(K, I)
        ms = med['vc_wpe_f32, K = %d, I = %d' % (K, I)]
        say('  K = %2d, I = %d: %7.3f GFLOP float64, %5.1f MB -> %9.4f ms = %7.1f GFLOP/s, %6.1f GB/s'
            % (K, I, ops / 1e9, nbytes / 1e6, ms, ops / ms / 1e6, nbytes / ms / 1e6))
    if a.kernels_only:
        return finish()

    # ---- the calls
    from ab_convert_batch import models
    dec, c = models()
    lens = [L] * B
    calls = {'convert_diff_batch': lambda: conversion.convert_diff_batch(dec, wav, lens, c),
             'convert_diff_batch(dereverb=True)': lambda: conversion.convert_diff_batch(dec, wav, lens, c, dereverb=True)}
    say('calls on 16 x 5 s, bf16 models (HIP events around one call)')
    for f in calls.values():
        f()
    med = report(interleaved(calls, a.reps, 1))
    k = list(calls)
    say('  dereverb=True adds %.3f ms to convert_diff_batch' % (med[k[1]] - med[k[0]]))
    finish()


if __name__ == '__main__':
    main()
