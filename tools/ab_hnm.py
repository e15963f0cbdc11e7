"""Timing of the harmonic-plus-noise vocoder (csrc/vc_hnm.hip behind audio_lib.envelope_batch / hnm_plan_batch / noise_batch /
hnm_synth_batch and conversion.convert_hnm_batch) on one MI355X: HIP events, arms interleaved, medians.

Kernels, 16 utterances x 1,001 frames x 201 bins (16 x 5 s at 16 kHz, hop 80), a speech-like contour (90 to 220 Hz gliding, a
fifth of the frames unvoiced):
  a float4 copy of the magnitude slab (torch's copy_); vc_env_cepstral_f32 at order 24 with 16 and with 0 iterations;
  vc_hnm_plan; vc_noise_init_f32; vc_hnm_noise_gain_f32; vc_hnm_synth_f32 with the cutoff at 4 kHz and at Nyquist; and the
  whole hnm_synth_batch chain (vc_stft_filter_f32's two launches included).  Event figures include the launch gap of a call
  from Python.
Calls, 16 x 5 s of synthetic audio, bf16 models:
  convert_batch and convert_pitch_batch(pitch='source') with 32 iterations of fast Griffin-Lim; convert_hnm_batch.

    python tools/ab_hnm.py --reps 7 --out profiles/hnm/ab_hnm.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_pitch import B, F, HOP, L, contour                          # noqa: E402  (the same sizes and contour)
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
    import _vc
    if not torch.cuda.is_available():
        raise SystemExit('ab_hnm needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t):
        med = {}
        for k, v in t.items():
            med[k] = float(np.median(v))
            say('  %-56s median %9.4f ms  (min %.4f, max %.4f, %d reps)' % (k, med[k], min(v), max(v), len(v)))
        return med

    # ---- kernels
    import hnm_ref
    rng = np.random.RandomState(1)
    env = hnm_ref.vowel(120.0, 1)[2]
    amp = torch.from_numpy((env[None, None, :] * np.exp(rng.normal(0.0, 0.3, (B, F, NB)))).astype(np.float32)).cuda()
    f0 = torch.from_numpy(contour(2)).cuda()
    d_nf = torch.full((B,), F, dtype=torch.int32, device='cuda')
    d_lens = torch.full((B,), HOP * (F - 1), dtype=torch.int32, device='cuda')
    plan = audio_lib._get_voc_plan(N_FFT, HOP, N_FFT)
    dst = torch.empty_like(amp)
    env_log, theta = audio_lib._envelope_launch(amp, d_nf, N_FFT, 24, 16, 1e-5)
    pl = audio_lib._hnm_plan_launch(f0, d_nf, SR, HOP, 40.0, SR / 4.0)
    cut4, cut8 = audio_lib.hnm_cutoff(4000.0, SR, N_FFT, 40.0), audio_lib.hnm_cutoff(8000.0, SR, N_FFT, 40.0)
    add, gain = audio_lib._hnm_noise_launch(plan, env_log, pl, d_nf, d_lens, cut4[1], 1.0, 1, None)
    inc = pl.inc.cpu().numpy().view(np.uint32).astype(np.float64)
    v = pl.voiced.cpu().numpy() != 0
    say('contour: %.0f %% of the frames voiced; %.1f harmonics per voiced frame below 4 kHz, %.1f below Nyquist'
        % (100 * v.mean(), ((cut4[0] - 1) // inc[v]).mean(), ((cut8[0] - 1) // inc[v]).mean()))
    lib = _vc.lib()
    gscale = 1.0 / np.sqrt(plan.window_sums()[1])

    def run_gain():
        _vc.check(lib.vc_hnm_noise_gain_f32(_vc.ptr(env_log), _vc.ptr(pl.voiced), _vc.ptr(d_nf), B, F, NB, cut4[1], gscale,
                                            _vc.ptr(gain), _vc.current_stream()))

    chain = lambda: audio_lib._hnm_chain(plan, amp, f0, d_nf, d_lens, SR, 24, 16, 1e-5, 40.0, SR / 4.0, cut4, 1.0, 1, None, True)
    arms = {'float4 copy of the magnitudes (torch copy_)': lambda: dst.copy_(amp),
            'vc_env_cepstral_f32, order 24, 16 iterations': lambda: audio_lib._envelope_launch(amp, d_nf, N_FFT, 24, 16, 1e-5),
            'vc_env_cepstral_f32, order 24, 0 iterations': lambda: audio_lib._envelope_launch(amp, d_nf, N_FFT, 24, 0, 1e-5),
            'vc_hnm_plan': lambda: audio_lib._hnm_plan_launch(f0, d_nf, SR, HOP, 40.0, SR / 4.0),
            'vc_noise_init_f32': lambda: audio_lib._noise_launch(d_lens, B, HOP * (F - 1), 1, None),
            'vc_hnm_noise_gain_f32': run_gain,
            'vc_hnm_synth_f32, cutoff 4 kHz, with add': lambda: audio_lib._hnm_synth_launch(plan, env_log, theta, pl, d_nf, cut4[0], add),
            'vc_hnm_synth_f32, cutoff at Nyquist': lambda: audio_lib._hnm_synth_launch(plan, env_log, theta, pl, d_nf, cut8[0], None),
            'hnm_synth_batch, every launch (noise branch included)': chain}
    say('kernels at %d x %d frames x %d bins (HIP events over %d back-to-back calls, launch gaps and allocations included)'
        % (B, F, NB, a.inner))
    report(interleaved(arms, a.reps, a.inner))

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
    kw = dict(n_iter=32, momentum=0.99, phase='device', seed=1)
    calls = {'convert_batch (32 iterations, momentum 0.99)': lambda: conversion.convert_batch(dec, wav, lens, c, **kw),
             "convert_pitch_batch(pitch='source') (the same vocoder)": lambda: conversion.convert_pitch_batch(dec, wav, lens, c, pitch='source', **kw),
             "convert_hnm_batch(pitch='source')": lambda: conversion.convert_hnm_batch(dec, wav, lens, c, seed=1)}
    r0, _, r2 = (f() for f in calls.values())
    assert torch.equal(r0.stft_pred, r2.stft_pred)
    say("calls on 16 x 5 s, bf16 models (HIP events around one call; convert_hnm_batch keeps convert_batch's spectra bit for bit); "
        '%.0f %% of the source frames voiced' % (100 * float((r2.f0_target > 0).float().mean())))
    for f in calls.values():
        f()
    med = report(interleaved(calls, a.reps, 1))
    k = list(calls)
    say('  convert_hnm_batch takes %.3f ms where convert_batch takes %.3f and convert_pitch_batch %.3f' % (med[k[2]], med[k[0]], med[k[1]]))
    finish()


if __name__ == '__main__':
    main()
