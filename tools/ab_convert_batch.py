"""Waveforms in, waveforms out: what a user of the public conversion calls gets, on one box, in one process,
interleaved (ABCABC...), with the shipped model sizes in bf16 (the reference's enc_14 encoder, a seeded decoder: the
repository carries no trained decoder), at 200 plain and at 32 momentum-0.99 Griffin-Lim iterations:

  (i)   a loop of the per-utterance calls as they stand: calc_MFCC_input + conversion2 per utterance (host numpy
        features, host stitch, host-drawn phase);
  (ii)  convert_batch(phase='numpy'): everything on the device except the reference's phase draws;
  (iii) convert_batch(phase='device').

for 16 utterances of 5 s and for a ragged set of 16 (1.5 .. 7 s).  Wall clock around a synchronised region after
warm-ups of every shape.  Then the three new kernels alone at the sizes of the 16 x 5 s batch: HIP events around
repeated launches, bytes moved from the shapes, and the fraction of the 6.3 TB/s a float4 copy reaches on this chip
(MI355X: 8 TB/s peak).  Prints one JSON line per measurement.
The event figures of the kernels include the launch gaps (about 8 us per launch from Python, whatever the size): for the
kernels' own durations run `rocprofv3 --kernel-trace --stats -- python tools/ab_convert_batch.py --kernels-only`.
python tools/ab_convert_batch.py [--reps 3] [--kernel-reps 200] [--kernels-only]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd')):
    sys.path.insert(0, p)
import numpy as np
import torch
import audio_lib
import conversion
from bench import synth_audio
from oracle import model_oracle as mo

HP = os.path.join(ROOT, 'speech-cloner_amd', 'hp')
HBM_COPY = 6.3e12          # bytes/s a float4 copy reaches


def models():
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    enc_cfg = json.load(open(os.path.join(HP, 'encoder_cfg_d.json')))
    enc_cfg.update(is_training=False, model_path=os.path.join(ROOT, 'tests', 'golden', 'enc_14_ckpt'), compute_dtype='bfloat16')
    dec_cfg = json.load(open(os.path.join(HP, 'decoder_cfg_d.json')))
    dec_cfg.update(is_training=False)
    c = json.load(open(os.path.join(HP, 'ds_dec_cfg_d.json')))
    c['hop_length'] = int(c['hop_length_ms'] * c['sample_rate'] / 1000.0)
    c['win_length'] = int(c['win_length_ms'] * c['sample_rate'] / 1000.0)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
        dec = decoder_specs(dec_cfg, None, enc)
    dec.store.load_dict(dict(mo.init_weights(dec_cfg, 'decoder', seed=2, perturb_bn=True)), strict=False)
    return dec, c


def fe_kwargs(c):
    return dict(sr=c['sample_rate'], pre_emphasis=c['pre_emphasis'], hop_length=c['hop_length'], win_length=c['win_length'],
                n_mels=c['n_mels'], n_mfcc=c['n_mfcc'], n_fft=c['n_fft'], window=c['window'],
                mfcc_normaleze_first_mfcc=c['mfcc_normaleze_first_mfcc'], mfcc_norm_factor=c['mfcc_norm_factor'],
                calc_mfcc_derivate=c['calc_mfcc_derivate'], M_dB_norm_factor=c['M_dB_norm_factor'],
                P_dB_norm_factor=c['P_dB_norm_factor'], mean_abs_amp_norm=c['mean_abs_amp_norm'], clip_output=c['clip_output'])


def loop_of_conversion2(dec, c, wav, lens, n_iter, momentum):
    out = []
    with contextlib.redirect_stdout(io.StringIO()):
        for b, L in enumerate(lens):
            mfcc, mel, stft = audio_lib.calc_MFCC_input(wav[b, :L], **fe_kwargs(c))
            out.append(conversion.conversion2(dec, mfcc, mel, stft, c, t_s=0, t_e=60, n_iter=n_iter, giffin_lim_input=False,
                                              momentum=momentum).y_wav_pred)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def events(fn, n):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n                  # s per launch, launch gaps included


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-reps', type=int, default=200)
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    dec, c = models()
    sets = {'16x5s': [80000] * 16,
            'ragged16': [int(16000 * s) for s in (1.5, 7.0, 3.2, 5.0, 2.1, 6.4, 4.4, 2.9, 5.6, 3.7, 1.8, 6.9, 4.1, 2.5, 5.2, 3.3)]}
    for name, lens in ({} if a.kernels_only else sets).items():
        wav = synth_audio(len(lens), max(lens), seed=300).numpy()
        for b, L in enumerate(lens):
            wav[b, L:] = 0.0
        seconds = sum(lens) / 16000.0
        for n_iter, momentum in ((200, 0.0), (32, 0.99)):
            forms = (('loop_conversion2', lambda: loop_of_conversion2(dec, c, wav, lens, n_iter, momentum)),
                     ('convert_batch_numpy', lambda: conversion.convert_batch(dec, wav, lens, c, n_iter=n_iter, momentum=momentum,
                                                                              phase='numpy')),
                     ('convert_batch_device', lambda: conversion.convert_batch(dec, wav, lens, c, n_iter=n_iter, momentum=momentum,
                                                                               phase='device')))
            for _, fn in forms:                                # warm-up: every shape of every form
                fn()
                fn()
            t = {k: [] for k, _ in forms}
            for _ in range(a.reps):
                for k, fn in forms:
                    t[k].append(wall(fn))
            for k, _ in forms:
                best, med = min(t[k]), sorted(t[k])[len(t[k]) // 2]
                print(json.dumps(dict(what='wall', set=name, n_iter=n_iter, momentum=momentum, form=k, ms_min=round(1e3 * best, 2),
                                      ms_median=round(1e3 * med, 2), all_ms=[round(1e3 * v, 2) for v in t[k]],
                                      audio_seconds=seconds, x_realtime=round(seconds / med, 1))), flush=True)

    # ---- the three kernels alone, 16 x 5 s: 1001 frames -> 1200, N = 3, 80 windows
    plan = conversion.convert_plan([80000] * 16, c, 0, 60, True)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    win, utt, clip, nout = dev(plan.win_tab), dev(plan.utt_tab), dev(plan.n_clip), dev(plan.n_out)
    g = torch.Generator().manual_seed(1)
    for C in (80, 201):
        src = torch.rand((16, 1001, C), generator=g).cuda()
        out = torch.empty((plan.W, 400, C), device='cuda')
        s = events(lambda: conversion.cut_windows(src, win, clip, 400, out=out), a.kernel_reps)
        # valid rows read + every row written
        nbytes = 4 * C * (int(sum(min(max(int(plan.n_clip[u]) - f0, 0), 400) for u, f0 in plan.win_tab)) + plan.W * 400)
        print(json.dumps(dict(what='kernel', kernel='vc_cut_windows', C=C, us=round(1e6 * s, 2), MB=round(nbytes / 1e6, 2),
                              TBps=round(nbytes / s / 1e12, 3), frac_of_copy_rate=round(nbytes / s / HBM_COPY, 3))), flush=True)
    for C, fused in ((80, False), (61, False), (201, False), (201, True)):
        y = torch.rand((plan.W, 400, C), generator=g).cuda()
        out = torch.empty((16, plan.Fout, C), device='cuda')
        amp = torch.empty_like(out) if fused else None
        s = events(lambda: conversion.compound_stitch(y, utt, plan.Fout, P_dB_norm_factor=0.01 if fused else None, out=out, amp=amp),
                   a.kernel_reps)
        nbytes = 4 * C * 16 * plan.Fout * (3 if fused else 2)
        print(json.dumps(dict(what='kernel', kernel='vc_compound_stitch' + ('+amp' if fused else ''), C=C, us=round(1e6 * s, 2),
                              MB=round(nbytes / 1e6, 2), TBps=round(nbytes / s / 1e12, 3),
                              frac_of_copy_rate=round(nbytes / s / HBM_COPY, 3))), flush=True)
    for F in (1200, 1000):
        ph = torch.empty((16, F, 201), device='cuda')
        nf = dev(np.full(16, F, np.int32))
        s = events(lambda: audio_lib.phase_init(nf, F, 201, seed=1, out=ph), a.kernel_reps)
        nbytes = 4 * 201 * 16 * F
        print(json.dumps(dict(what='kernel', kernel='vc_phase_init', frames=F, us=round(1e6 * s, 2), MB=round(nbytes / 1e6, 2),
                              TBps=round(nbytes / s / 1e12, 3), frac_of_copy_rate=round(nbytes / s / HBM_COPY, 3))), flush=True)
    t0 = time.perf_counter()
    for _ in range(5):
        ph = np.zeros((16, 1000, 201), np.float32)
        for b in range(16):
            ph[b] = (np.pi * np.random.rand(201, 1000)).T
    print(json.dumps(dict(what='host', item='numpy phase draws 16 x 1000 x 201 (griffin_lim_batch default)',
                          ms=round((time.perf_counter() - t0) / 5 * 1e3, 2))), flush=True)


if __name__ == '__main__':
    main()
