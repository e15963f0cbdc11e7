"""The device resampler (audio_lib.resample_batch, csrc/vc_resample.hip) against what a user has without it, on one
box, in one process, interleaved (ABAB...), medians of HIP-event times:

  kernel  resample_batch on a cuda batch (one launch);
  (a)     the parent commit's route: scipy.signal.resample_poly per utterance on the host with the same taps, plus the
          upload of the result (wall clock, synchronised);
  (b)     the same polyphase product with torch ops on the GPU: ONE strided conv1d whose output channels are the `up`
          phases (each channel's taps shifted by its phase's input offset), then a transpose to interleave them.

Shapes: 32 x 4 s and 16 x 5 s from 44.1 kHz and 48 kHz to 16 kHz, both presets.  For each: microseconds, GB/s of the
bytes the algorithm must move (input + output once) against 8 TB/s, GFLOP/s of 2 x outputs x taps per output against
the 157 TFLOP/s float32 peak, which of the two bounds the case, and the fraction of that bound reached.  The event
times include the launch gap of a call from Python (several microseconds); the kernel's own duration comes from
`rocprofv3 --kernel-trace --stats -- python tools/ab_resample.py --kernel-only`.
--convert adds convert_batch 16 x 5 s fed at 48 kHz against the same audio fed at 16 kHz (the resampler's share).
python tools/ab_resample.py [--reps 30] [--kernel-only] [--no-torch] [--convert]"""
import argparse
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)
import numpy as np
import torch
import audio_lib

HBM_PEAK, F32_PEAK = 8.0e12, 157.0e12


def event_us(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def torch_polyphase(sr_in, sr_out, res_type):
    """(weight [up, 1, ntap + shift_max], lead) for F.conv1d(x padded by `lead` zeros in front, weight, stride=down)."""
    up, down, half, g = audio_lib.resample_taps(sr_in, sr_out, res_type)
    jhi, jlo = half // up, -((half + up - 1) // up)
    ntap = jhi - jlo + 1
    shift = [(s * down) // up for s in range(up)]
    w = np.zeros((up, 1, ntap + max(shift)), np.float32)
    for s in range(up):
        p = (s * down) % up
        k = p + (jhi - np.arange(ntap)) * up
        ok = np.abs(k) <= half
        w[s, 0, shift[s] + np.arange(ntap)[ok]] = g[k[ok] + half]
    return torch.from_numpy(w).cuda(), jhi, up, down, ntap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--convert', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ab_resample needs a GPU')
    from scipy import signal
    for B, secs in ((32, 4), (16, 5)):
        for sr_in in (44100, 48000):
            L = secs * sr_in
            wav = np.random.RandomState(B).uniform(-0.5, 0.5, (B, L)).astype(np.float32)
            d_wav = torch.from_numpy(wav).cuda()
            for res_type in ('kaiser_best', 'kaiser_fast'):
                up, down, half, g = audio_lib.resample_taps(sr_in, 16000, res_type)
                n_out = audio_lib.resample_len(L, sr_in, 16000)
                out = torch.empty((B, n_out), device='cuda')
                run = lambda: audio_lib.resample_batch(d_wav, None, sr_in=sr_in, sr_out=16000, res_type=res_type, out=out)
                run(); torch.cuda.synchronize()
                taps_per_out = (2 * half + 1) / up
                nbytes, flops = 4.0 * B * (L + n_out), 2.0 * B * n_out * taps_per_out
                t_floor = max(nbytes / HBM_PEAK, flops / F32_PEAK)
                bound = 'bytes' if nbytes / HBM_PEAK >= flops / F32_PEAK else 'flops'
                rec = dict(what='resample', B=B, seconds=secs, sr_in=sr_in, res_type=res_type, up=up, down=down,
                           taps_per_output=round(taps_per_out, 1), MB=round(nbytes / 1e6, 2), GFLOP=round(flops / 1e9, 3), bound=bound)
                if args.kernel_only:
                    for _ in range(args.reps):
                        run()
                    torch.cuda.synchronize()
                    print(json.dumps(rec)); sys.stdout.flush()
                    continue
                use_torch = not args.no_torch
                if use_torch:
                    w, jhi, _, _, ntap = torch_polyphase(sr_in, 16000, res_type)
                    n_i = (n_out + up - 1) // up
                    need = (n_i - 1) * down + w.shape[2]
                    xp = torch.zeros((B, 1, max(need, jhi + L)), device='cuda')

                    def run_torch():
                        xp[:, 0, jhi:jhi + L] = d_wav
                        y = torch.nn.functional.conv1d(xp[:, :, :need], w, stride=down)          # [B, up, n_i]
                        return y.transpose(1, 2).reshape(B, -1)[:, :n_out]
                    yt = run_torch(); torch.cuda.synchronize()
                    rec['torch_vs_kernel_max_abs'] = float((yt - out).abs().max())
                ker, tor = [], []
                for _ in range(args.reps):                                   # interleaved
                    ker += event_us(run, 1)
                    if use_torch:
                        tor += event_us(run_torch, 1)
                host = []
                for _ in range(3):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    ys = np.stack([signal.resample_poly(wav[b].astype(np.float64), up, down, window=g / up).astype(np.float32) for b in range(B)])
                    torch.from_numpy(ys).cuda(); torch.cuda.synchronize()
                    host.append(1e6 * (time.perf_counter() - t0))
                us = float(np.median(ker))
                rec.update(us=round(us, 1), us_min=round(min(ker), 1), GBps=round(nbytes / us / 1e3, 1), GFLOPs=round(flops / us / 1e3, 1),
                           fraction_of_bound=round(t_floor * 1e6 / us, 4), host_scipy_plus_upload_us=round(float(np.median(host)), 0))
                if use_torch:
                    rec['torch_conv1d_us'] = round(float(np.median(tor)), 1)
                print(json.dumps(rec)); sys.stdout.flush()
    if args.convert and not args.kernel_only:
        import conversion
        from ab_convert_batch import models
        dec, c = models()
        B, secs = 16, 5
        w48 = np.random.RandomState(1).uniform(-0.3, 0.3, (B, secs * 48000)).astype(np.float32)
        d48 = torch.from_numpy(w48).cuda()
        d16 = audio_lib.resample_batch(d48, None, sr_in=48000, sr_out=16000)[0]
        f48 = lambda: conversion.convert_batch(dec, d48, None, c, n_iter=32, momentum=0.99, wav_sr=48000)
        f16 = lambda: conversion.convert_batch(dec, d16, None, c, n_iter=32, momentum=0.99)
        for f in (f48, f16, f48, f16):
            f()
        torch.cuda.synchronize()
        t48, t16 = [], []
        for _ in range(10):
            for f, acc in ((f48, t48), (f16, t16)):
                torch.cuda.synchronize(); t0 = time.perf_counter(); f(); torch.cuda.synchronize()
                acc.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps(dict(what='convert_batch 16 x 5 s, bf16, 32 iterations momentum 0.99', ms_48k_in=round(float(np.median(t48)), 3),
                              ms_16k_in=round(float(np.median(t16)), 3))))


if __name__ == '__main__':
    main()
