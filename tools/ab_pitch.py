"""Timing of pitch conversion (csrc/vc_pitch.hip behind conversion.psola_plan_batch / pitch_shift_batch /
convert_pitch_batch) on one MI355X: HIP events, arms interleaved, medians.

Kernels, 16 utterances x 80,000 samples (16 x 5 s at 16 kHz), 1,001 frames of tables:
  a float4 copy of the same slab (torch's copy_); vc_psola_plan for a speech-like contour (90 to 220 Hz gliding, a fifth of
  the frames unvoiced) at ratio 1.25, and for the shortest period the launch takes (16 samples: 5,000 marks per utterance);
  vc_psola_ola_f32 on the first plan (about 30 staged grains per tile, 2 to 3 covering a sample) and on the second (192
  staged grains per tile: the longest list a tile can have).  Event figures include the launch gap of a call from Python.
Calls, 16 x 5 s of synthetic audio, bf16 models, 32 iterations of fast Griffin-Lim:
  convert_batch; convert_pitch_batch(pitch=1.0): the price of the feature (tracker, tables, plan, overlap-add);
  convert_pitch_batch(pitch='source'): what tracking the input as well adds.

    python tools/ab_pitch.py --reps 7 --out profiles/pitch/ab_pitch.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_pitch.py --kernels-only --shape contour
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_warp import interleaved                                     # noqa: E402  (the same timing loops)

HBM_COPY = 6.3e12          # bytes/s a float4 copy reaches
B, L, HOP = 16, 80000, 80
F = 1 + L // HOP


def contour(seed):
    """[B, F] float32 Hz: a gliding fundamental per utterance, about a fifth of the frames unvoiced in stretches."""
    rng = np.random.RandomState(seed)
    t = np.arange(F) * HOP / 16000.0
    f0 = np.stack([rng.uniform(90.0, 220.0) * 2.0 ** (0.35 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t)) for _ in range(B)])
    for b in range(B):
        for s in rng.randint(0, F - 25, 8):
            f0[b, s:s + 25] = 0.0
    return f0.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50, help='back-to-back launches per kernel timing')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--shape', choices=('both', 'contour', 'period16'), default='both',
                    help='the kernel arms to run: under a kernel trace one shape a run keeps the per-kernel rows apart')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import conversion
    import _vc
    if not torch.cuda.is_available():
        raise SystemExit('ab_pitch needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t, nbytes=None):
        med = {}
        for k, v in t.items():
            med[k] = float(np.median(v))
            extra = ''
            if nbytes and k in nbytes:
                r = nbytes[k] / (med[k] * 1e-3)
                extra = '  %.1f MB, %.2f TB/s, %.0f %% of the copy rate' % (nbytes[k] / 1e6, r / 1e12, 100 * r / HBM_COPY)
            say('  %-52s median %9.4f ms  (min %.4f, max %.4f, %d reps)%s' % (k, med[k], min(v), max(v), len(v), extra))
        return med

    # ---- kernels
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((B, L), generator=g) - 0.5).cuda()
    dst, y = torch.empty_like(x), torch.empty_like(x)
    d_lens = torch.full((B,), L, dtype=torch.int32, device='cuda')
    per, rat = conversion.pitch_tables(torch.from_numpy(contour(2)).cuda(), 16000, ratio=1.25, hop_length=HOP)
    per16, rat1 = torch.full_like(per, 16 << 16), torch.full_like(rat, 65536)
    plan = conversion.psola_plan_batch(per, rat, d_lens, HOP, max_len=L)
    plan16 = conversion.psola_plan_batch(per16, rat1, d_lens, HOP, max_len=L)
    win = conversion.psola_window('cuda')
    say('plans: %.0f analysis and %.0f synthesis marks per utterance for the contour, %d for period 16'
        % (float(plan.n_a.float().mean()), float(plan.n_s.float().mean()), int(plan16.n_s[0])))
    lib = _vc.lib()

    def run_plan(p, r, o):
        _vc.check(lib.vc_psola_plan(_vc.ptr(p), _vc.ptr(r), _vc.ptr(d_lens), B, L, F, HOP, _vc.ptr(o.n_a), _vc.ptr(o.n_s), _vc.ptr(o.a),
                                    _vc.ptr(o.s), _vc.ptr(o.src), _vc.ptr(o.h), _vc.current_stream()))

    def run_ola(o):
        _vc.check(lib.vc_psola_ola_f32(_vc.ptr(x), _vc.ptr(d_lens), _vc.ptr(o.n_s), _vc.ptr(o.s), _vc.ptr(o.src), _vc.ptr(o.h), _vc.ptr(win),
                                       B, L, 0.5, _vc.ptr(y), _vc.current_stream()))

    slab = 4 * B * L
    arms = {'float4 copy (torch copy_)': lambda: dst.copy_(x),
            'vc_psola_plan, speech-like contour x 1.25': lambda: run_plan(per, rat, plan),
            'vc_psola_plan, period 16 (5,000 marks)': lambda: run_plan(per16, rat1, plan16),
            'vc_psola_ola_f32, speech-like contour x 1.25': lambda: run_ola(plan),
            'vc_psola_ola_f32, period 16 (192 grains a tile)': lambda: run_ola(plan16)}
    # bytes: one waveform read, one written (the gathers of overlapping grains hit the same lines)
    nbytes = {'float4 copy (torch copy_)': 2 * slab, 'vc_psola_ola_f32, speech-like contour x 1.25': 2 * slab,
              'vc_psola_ola_f32, period 16 (192 grains a tile)': 2 * slab}
    if a.shape != 'both':
        skip = 'period 16' if a.shape == 'contour' else 'contour'
        arms = {k: v for k, v in arms.items() if skip not in k}
    say('kernels at %d x %d samples, %d frames (HIP events over %d back-to-back calls, launch gaps included)' % (B, L, F, a.inner))
    report(interleaved(arms, a.reps, a.inner), nbytes)

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
    calls = {'convert_batch': lambda: conversion.convert_batch(dec, wav, lens, c, **kw),
             'convert_pitch_batch(pitch=1.0)': lambda: conversion.convert_pitch_batch(dec, wav, lens, c, pitch=1.0, **kw),
             "convert_pitch_batch(pitch='source')": lambda: conversion.convert_pitch_batch(dec, wav, lens, c, pitch='source', **kw)}
    r0, r1, r2 = (f() for f in calls.values())
    assert torch.equal(r0.stft_pred, r1.stft_pred) and torch.equal(r1.plan.s, r1.plan.a) and torch.equal(r1.f0_pred, r2.f0_pred)
    say('calls on 16 x 5 s, bf16 models, 32 iterations at momentum 0.99 (HIP events around one call; pitch=1.0 keeps '
        "convert_batch's spectra bit for bit and copies the analysis marks); %.0f %% of the converted frames voiced, %.0f synthesis marks "
        'per utterance' % (100 * float((r1.f0_pred > 0).float().mean()), float(r1.plan.n_s.float().mean())))
    for f in calls.values():
        f()
    med = report(interleaved(calls, a.reps, 1))
    say('  the feature costs %.3f ms on %.3f (%.1f %%); tracking the input as well adds %.3f ms'
        % (med['convert_pitch_batch(pitch=1.0)'] - med['convert_batch'], med['convert_batch'],
           100 * (med['convert_pitch_batch(pitch=1.0)'] / med['convert_batch'] - 1),
           med["convert_pitch_batch(pitch='source')"] - med['convert_pitch_batch(pitch=1.0)']))
    finish()


if __name__ == '__main__':
    main()
