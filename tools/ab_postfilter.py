"""Timing of the postfilters (csrc/vc_postfilter.hip behind speech-cloner_amd/postfilter.py and
conversion.convert_postfilter_batch) on one MI355X: HIP events, arms interleaved, medians, with the spread.

Kernels, 16 utterances x 1,001 frames x 201 bins (16 x 5 s of stft_pred), outputs allocated once:
  vc_traj_stats_f32 and vc_ms_stats_f32 against a float4 copy of the bytes they read (the statistics they write are small);
  vc_gv_filter_f32 and vc_ms_filter_f32 against a float4 copy of the same bytes in and out (12.9 MB each way).
  Event figures include the launch gap of a call from Python.
Calls, 16 x 5 s of synthetic audio, bf16 models, 32 iterations at momentum 0.99:
  convert_batch; convert_postfilter_batch in the modes 'ms', 'gv' and 'ms+gv' with the model's tables uploaded once.

    python tools/ab_postfilter.py --reps 7 --out profiles/postfilter/ab_postfilter.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_warp import interleaved                                     # noqa: E402  (the same timing loops)

B, L, HOP, C = 16, 80000, 80, 201
F = 1 + L // HOP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50, help='back-to-back launches per kernel timing')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import _vc
    import conversion
    import postfilter
    if not torch.cuda.is_available():
        raise SystemExit('ab_postfilter needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t, nbytes=None, copies=None):
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, v in t.items():
            extra = ''
            if nbytes and k in nbytes:
                extra = '  %.1f MB, %.2f TB/s' % (nbytes[k] / 1e6, nbytes[k] / (med[k] * 1e-3) / 1e12)
                if copies and k in copies:
                    extra += ', %.2f x its copy' % (med[k] / med[copies[k]])
            say('  %-52s median %9.4f ms  (min %.4f, max %.4f, spread %.1f %%, %d reps)%s'
                % (k, med[k], min(v), max(v), 100 * (max(v) - min(v)) / med[k], len(v), extra))
        return med

    # ---- kernels: a smoothed random walk per bin, so that the logarithms and exponentials see ordinary values
    g = torch.Generator().manual_seed(1)
    z = torch.randn((B, F + 2, C), generator=g)
    x = (0.45 + 0.05 * (z[:, 2:] + z[:, 1:-1] + z[:, :-2])).cuda().contiguous()
    d_nf = torch.full((B,), F, dtype=torch.int32, device='cuda')
    lib, st = _vc.lib(), _vc.current_stream
    stats = postfilter.traj_stats_batch(x, d_nf)
    ms = postfilter.ms_stats_batch(x, d_nf, stats)
    model = postfilter.fit([(x, d_nf)], [(0.8 * x + 0.09, d_nf)])
    tables = postfilter.upload(model, 0.85)
    y = torch.empty_like(x)
    hi = 20.0 * np.log(10.0) / 20.0
    spec = 4 * B * F * C
    src1, dst1 = torch.empty(spec // 4, device='cuda'), torch.empty(spec // 4, device='cuda')
    src_h, dst_h = torch.empty(spec // 8, device='cuda'), torch.empty(spec // 8, device='cuda')
    P = _vc.ptr
    arms = {'float4 copy, 12.9 MB in and out': lambda: dst1.copy_(src1),
            'float4 copy, 6.4 MB in and out': lambda: dst_h.copy_(src_h),
            'vc_traj_stats_f32': lambda: _vc.check(lib.vc_traj_stats_f32(P(x), P(d_nf), B, F, C, P(stats), st())),
            'vc_ms_stats_f32': lambda: _vc.check(lib.vc_ms_stats_f32(P(x), P(d_nf), P(stats), B, F, C, P(ms), st())),
            'vc_gv_filter_f32': lambda: _vc.check(lib.vc_gv_filter_f32(P(x), P(d_nf), P(stats), P(tables.gv_t), B, F, C, 1.0, 4.0, P(y), st())),
            'vc_ms_filter_f32': lambda: _vc.check(lib.vc_ms_filter_f32(P(x), P(d_nf), P(stats), P(tables.coef), B, F, C, -hi, hi, P(y), st()))}
    nbytes = {'float4 copy, 12.9 MB in and out': 2 * spec, 'float4 copy, 6.4 MB in and out': spec, 'vc_traj_stats_f32': spec,
              'vc_ms_stats_f32': spec, 'vc_gv_filter_f32': 2 * spec, 'vc_ms_filter_f32': 2 * spec}
    copies = {'vc_traj_stats_f32': 'float4 copy, 6.4 MB in and out', 'vc_ms_stats_f32': 'float4 copy, 6.4 MB in and out',
              'vc_gv_filter_f32': 'float4 copy, 12.9 MB in and out', 'vc_ms_filter_f32': 'float4 copy, 12.9 MB in and out'}
    say('kernels at %d x %d frames x %d bins (HIP events over %d back-to-back calls, launch gaps included; the statistics launches '
        'read 12.9 MB, their copy moves the same bytes as 6.4 MB in and 6.4 MB out)' % (B, F, C, a.inner))
    report(interleaved(arms, a.reps, a.inner), nbytes, copies)

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
    post = lambda mode: (lambda: conversion.convert_postfilter_batch(dec, wav, lens, c, model=tables, mode=mode, **kw))
    calls = {'convert_batch': lambda: conversion.convert_batch(dec, wav, lens, c, **kw),
             "convert_postfilter_batch, mode 'ms'": post('ms'), "convert_postfilter_batch, mode 'gv'": post('gv'),
             "convert_postfilter_batch, mode 'ms+gv'": post('ms+gv')}
    r0, r1 = calls['convert_batch'](), calls["convert_postfilter_batch, mode 'ms'"]()
    assert torch.equal(r0.stft_pred, r1.stft_raw) and torch.isfinite(r1.y_wav_pred).all()
    say('calls on 16 x 5 s, bf16 models, 32 iterations at momentum 0.99 (HIP events around one call); the model is a stand-in '
        'fitted on random trajectories: the timing does not depend on it')
    med = report(interleaved(calls, a.reps, 1))
    for k in list(calls)[1:]:
        say('  %s adds %.3f ms (%.1f %%) to convert_batch' % (k, med[k] - med['convert_batch'],
                                                               100 * (med[k] - med['convert_batch']) / med['convert_batch']))
    finish()


if __name__ == '__main__':
    main()
