"""Timing of duration conversion (csrc/vc_warp.hip behind conversion.duration_map_batch / time_warp_batch /
convert_duration_batch) on one MI355X: HIP events, arms interleaved, medians.

Kernels, 16 utterances x 1,200 output frames x 201 bins (the stitched spectrum of 16 x 5 s):
  vc_time_warp along the identity map (whole-frame positions: one source row per output row), along a 0.8 x map from 1,500
  frames (fractional positions: two source rows per output row), the latter with the fused magnitude; vc_compound_stitch
  at the same output shape, with and without its magnitude; a float4 copy of the same slab (torch's copy_); and
  vc_duration_map for a table of 150 segments per utterance.  Event figures include the launch gap of a call from Python.
Calls, 16 x 5 s of synthetic audio, bf16 models, 32 iterations of fast Griffin-Lim:
  convert_batch; convert_duration_batch(rate=1.0): the price of the feature; convert_duration_batch(segments='decode',
  ratio=ones): what the decoding adds.

    python tools/ab_warp.py --reps 7 --out profiles/duration/ab_warp.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_warp.py --kernels-only
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

HBM_COPY = 6.3e12          # bytes/s a float4 copy reaches
B, FW, C = 16, 1200, 201


def timed(fn, n):
    """ms per call over n back-to-back calls between two HIP events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(arms, reps, inner):
    import torch
    for fn in arms.values():                                        # warm-up
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn, inner))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50, help='back-to-back launches per kernel timing')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import conversion
    if not torch.cuda.is_available():
        raise SystemExit('ab_warp needs a GPU')
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
            say('  %-46s median %9.4f ms  (min %.4f, max %.4f, %d reps)%s' % (k, med[k], min(v), max(v), len(v), extra))
        return med

    # ---- kernels
    g = torch.Generator().manual_seed(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lens_id, lens_sq = dev(np.full(B, FW, np.int32)), dev(np.full(B, 1500, np.int32))
    x_id, x_sq = torch.rand((B, FW, C), generator=g).cuda(), torch.rand((B, 1500, C), generator=g).cuda()
    one = lambda n: (np.zeros((B, 1), np.int32), np.full((B, 1), n, np.int32), np.ones(B, np.int32))
    m_id = conversion.duration_map_batch(*one(FW), lens_id, ratio=1.0, max_frames=FW)
    m_sq = conversion.duration_map_batch(*one(1500), lens_sq, ratio=0.8, max_frames=FW)
    assert m_id.n_out.tolist() == [FW] * B and m_sq.n_out.tolist() == [FW] * B and int((m_sq.pos & 65535).ne(0).sum()) > B * FW // 2
    plan = conversion.convert_plan([80000] * B, dict(n_timesteps=400, hop_length=80, sample_rate=16000), 0, 60, True)
    assert plan.Fout == FW
    utt = dev(plan.utt_tab)
    y = torch.rand((plan.W, 400, C), generator=g).cuda()
    out, amp, dst = (torch.empty((B, FW, C), device='cuda') for _ in range(3))
    import _vc

    def warp(x, m, d_lens, norm):
        _vc.check(_vc.lib().vc_time_warp(_vc.ptr(x), _vc.ptr(m.pos), _vc.ptr(m.n_out), _vc.ptr(d_lens), B, x.shape[1], FW, C, 0, _vc.ptr(out),
                                         _vc.ptr(amp) if norm else None, norm, _vc.current_stream()))

    rng = np.random.RandomState(2)
    K = 150
    cuts = np.stack([np.sort(rng.choice(np.arange(1, FW), K - 1, replace=False)) for _ in range(B)])
    start = dev(np.concatenate([np.zeros((B, 1), np.int64), cuts], 1).astype(np.int32))
    end = dev(np.concatenate([cuts, np.full((B, 1), FW)], 1).astype(np.int32))
    n_seg, labels = dev(np.full(B, K, np.int32)), dev(rng.randint(0, 61, (B, K)).astype(np.int32))
    ratio = dev(rng.uniform(0.6, 1.6, 61).astype(np.float32))
    slab = 4 * B * FW * C
    arms = {'float4 copy (torch copy_)': lambda: dst.copy_(x_id),
            'vc_compound_stitch': lambda: conversion.compound_stitch(y, utt, FW, out=out),
            'vc_compound_stitch + magnitude': lambda: conversion.compound_stitch(y, utt, FW, P_dB_norm_factor=0.01, out=out, amp=amp),
            'vc_time_warp, identity map': lambda: warp(x_id, m_id, lens_id, 0.0),
            'vc_time_warp, 0.8 x (two rows)': lambda: warp(x_sq, m_sq, lens_sq, 0.0),
            'vc_time_warp, 0.8 x + magnitude': lambda: warp(x_sq, m_sq, lens_sq, 0.01),
            'vc_duration_map, 150 segments (Python call)': lambda: conversion.duration_map_batch(start, end, n_seg, lens_id, labels=labels,
                                                                                               ratio=ratio, max_frames=2048)}
    # bytes: the slab written, the source rows an utterance's output touches read once (1,200 / 1,500 rows), magnitude = one more slab
    nbytes = {'float4 copy (torch copy_)': 2 * slab, 'vc_compound_stitch': 2 * slab, 'vc_compound_stitch + magnitude': 3 * slab,
              'vc_time_warp, identity map': 2 * slab, 'vc_time_warp, 0.8 x (two rows)': slab + slab * 1500 // FW,
              'vc_time_warp, 0.8 x + magnitude': 2 * slab + slab * 1500 // FW}
    say('kernels at %d x %d x %d (HIP events over %d back-to-back calls, launch gaps included)' % (B, FW, C, a.inner))
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
    lens = [80000] * B
    wav = synth_audio(B, max(lens), seed=300).cuda()
    kw = dict(n_iter=32, momentum=0.99, phase='device', seed=1)
    ones = torch.ones(61, device='cuda')
    calls = {'convert_batch': lambda: conversion.convert_batch(dec, wav, lens, c, **kw),
             'convert_duration_batch(rate=1.0)': lambda: conversion.convert_duration_batch(dec, wav, lens, c, rate=1.0, **kw),
             "convert_duration_batch(segments='decode')": lambda: conversion.convert_duration_batch(dec, wav, lens, c, ratio=ones,
                                                                                                   max_frames=FW, **kw)}
    r0, r1, r2 = (f() for f in calls.values())
    assert torch.equal(r0.y_wav_pred, r1.y_wav_pred) and torch.equal(r0.stft_pred, r2.stft_pred) and r2.flags.tolist() == [0] * B
    say('calls on 16 x 5 s, bf16 models, 32 iterations at momentum 0.99 (HIP events around one call; rate=1.0 returns '
        "convert_batch's waveform bit for bit, ratio=ones its spectra); %.0f decoded segments per utterance" % float(r2.seg.n_seg.float().mean()))
    for f in calls.values():
        f()
    med = report(interleaved(calls, a.reps, 1))
    say('  the feature costs %.3f ms on %.3f (%.1f %%); decoding adds %.3f ms'
        % (med['convert_duration_batch(rate=1.0)'] - med['convert_batch'], med['convert_batch'],
           100 * (med['convert_duration_batch(rate=1.0)'] / med['convert_batch'] - 1),
           med["convert_duration_batch(segments='decode')"] - med['convert_duration_batch(rate=1.0)']))
    finish()


if __name__ == '__main__':
    main()
