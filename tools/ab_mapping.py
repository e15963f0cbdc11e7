"""Measurements of the spectral-mapping launches (csrc/vc_mapping.hip) on one MI355X.

Input: random features and models -- the figures are times, not scores.

  default        HIP-event times of one EM iteration (prepare, accumulate + reduce, update) on 16 pairs x 1,000 frames, D = 48,
                 M = 32 and 256; of the map launch; of the MLPG launch at 16 x 1,001 x 24 in float64 and, as an A/B, with
                 float32 arithmetic in the same order (a second build of the library with -DVC_MLPG_REAL=float, made by
                 --build-variant and never shipped); of the gain launch; wall times of convert_gmm_diff_batch against
                 convert_diff_batch at 16 x 5 s; and of mapping.fit against tests/mapping_ref.py on the host
  --build-variant  compile the float32-MLPG variant into tools/_build/ (needs the objects of a built tree) and exit
  --kernel-only  a few fits and conversions and nothing else: for a kernel trace

    python tools/ab_mapping.py --build-variant
    python tools/ab_mapping.py --reps 9 --out profiles/mapping/ab_mapping.log
"""
import argparse
import ctypes as C
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12        # MI355X: 8 TB/s
VARIANT = os.path.join(ROOT, 'tools', '_build', 'libvc_hip_mlpg_f32.so')


def build_variant():
    csrc = os.path.join(ROOT, 'speech-cloner_amd', 'csrc')
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    obj = os.path.join(os.path.dirname(VARIANT), 'vc_mapping_f32.o')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '-O3', '-fno-slp-vectorize', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I',
                           os.path.join(ROOT, 'include'), '-I', csrc, '-DVC_MLPG_REAL=float', '-c', os.path.join(csrc, 'vc_mapping.hip'),
                           '-o', obj])
    others = [o for o in sorted(glob.glob(os.path.join(csrc, '*.o'))) if os.path.basename(o) != 'vc_mapping.o']
    if not others:
        raise SystemExit('no objects in %s: build the library first' % csrc)
    subprocess.check_call([hipcc, '-shared', '-fPIC', '--offload-arch=gfx950', obj] + others + ['-o', VARIANT])
    print('built', VARIANT)


def event_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), min(out), max(out)


def wall_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--build-variant', action='store_true')
    a = ap.parse_args()
    if a.build_variant:
        build_variant()
        return
    import torch
    import _vc
    import conversion
    import mapping
    import mapping_cases as mc
    import mapping_ref as mr
    if not torch.cuda.is_available():
        raise SystemExit('ab_mapping needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    B, F, D = 16, 1000, 48
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    fa, fb = cuda(rng.standard_normal((B, F, D)).astype(np.float32)), cuda(rng.standard_normal((B, F, D)).astype(np.float32))
    lens = [F] * B
    d_len = torch.tensor(lens, dtype=torch.int32, device='cuda')
    if a.kernel_only:
        for _ in range(a.reps):
            model, _ = mapping.fit(fa, lens, fb, lens, n_components=32, n_iter=3)
            mapping.convert_cepstra_batch(model, fa[:, :, :D // 2].contiguous(), lens)
        torch.cuda.synchronize()
        return
    floor = torch.full((D,), 1e-3, device='cuda')
    for M in (32, 256):
        m = mr.random_model(M, D, seed=1, spread=0.5)
        model = mapping.JDGMM(*(cuda(m[k]) for k in mr.FIELDS))
        tab = mapping._prepare_launch(model)
        ws = torch.empty(mapping.workspace_size(M, D), dtype=torch.uint8, device='cuda')
        st = mapping._accumulate_launch(fa, fb, d_len, d_len, None, None, tab, M, ws=ws)
        say('one EM iteration, %d pairs x %d cells, D = %d, M = %d (median / min / max of %d, HIP events, ms):' % (B, F, D, M, a.reps))
        t = {'prepare': event_ms(lambda: mapping._prepare_launch(model), a.reps),
             'accumulate': event_ms(lambda: mapping._accumulate_launch(fa, fb, d_len, d_len, None, None, tab, M, ws=ws), a.reps),
             'update': event_ms(lambda: mapping._update_launch(st, model, floor, floor, 0.99, 1.0), a.reps),
             'map': event_ms(lambda: mapping._map_launch(fa, d_len, tab, M, 0), a.reps)}
        for k, v in t.items():
            say('  %-10s %.4f / %.4f / %.4f' % (k, *v))
        chunks = (M + 63) // 64
        n = B * F
        must = chunks * n * 2 * D * 4 + 2 * mapping.workspace_size(M, D)
        flops = chunks * n * M * 9 * D + n * M * 8 * D * 2          # the likelihoods once per chunk (float32) + the float64 folds as 2
        say('  accumulate must move %.1f MB (%.2f %% of the HBM line at its time) and do %.2f GFLOP; map must move %.1f MB (%.2f %%)'
            % (must / 1e6, 100 * must / HBM_BYTES_PER_S / (t['accumulate'][0] * 1e-3), flops / 1e9, 4 * n * D * 4 / 1e6,
               100 * 4 * n * D * 4 / HBM_BYTES_PER_S / (t['map'][0] * 1e-3)))
    # MLPG: float64 against float32 in the same order
    Bm, Fm, n = 16, 1001, 24
    P = cuda(rng.uniform(0.5, 5.0, (Bm, Fm, 2 * n)).astype(np.float32))
    R = (P * cuda(rng.standard_normal((Bm, Fm, 2 * n)).astype(np.float32))).contiguous()
    lm = torch.full((Bm,), Fm, dtype=torch.int32, device='cuda')
    t64 = event_ms(lambda: mapping._mlpg_launch(P, R, lm), a.reps)
    y64 = mapping._mlpg_launch(P, R, lm).y
    say('vc_mlpg_f32, %d x %d x %d, float64: %.4f / %.4f / %.4f ms: %.1f ns per row of the %d-row chain (forward and back)'
        % (Bm, Fm, n, *t64, 1e6 * t64[0] / (2 * Fm), 2 * Fm))
    if os.path.exists(VARIANT):
        h = C.CDLL(VARIANT)
        h.vc_mlpg_f32.restype, h.vc_mlpg_f32.argtypes = _vc._SIGS['vc_mlpg_f32']
        h.vc_mlpg_workspace_size.restype, h.vc_mlpg_workspace_size.argtypes = _vc._SIGS['vc_mlpg_workspace_size']
        need = h.vc_mlpg_workspace_size(Bm, Fm, n)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        y32 = torch.empty((Bm, Fm, n), dtype=torch.float32, device='cuda')
        fl = torch.empty((Bm,), dtype=torch.int32, device='cuda')

        def f32():
            rc = h.vc_mlpg_f32(_vc.ptr(P), _vc.ptr(R), _vc.ptr(lm), Bm, Fm, n, _vc.ptr(y32), _vc.ptr(fl), _vc.ptr(ws), need, _vc.current_stream())
            assert rc == 0, rc
        t32 = event_ms(f32, a.reps)
        say('the same with float32 arithmetic in the same order (variant build): %.4f / %.4f / %.4f ms; float64 costs x %.2f; the '
            'float32 trajectory is up to %.2e from the float64 one (values of order 1)' % (*t32, t64[0] / t32[0], float((y32 - y64).abs().max())))
    else:
        say('no float32 variant at %s (python tools/ab_mapping.py --build-variant on a built tree)' % os.path.relpath(VARIANT, ROOT))
    # the gain
    import evaluation
    cfg = mc.CFG
    i0, w = mapping.gain_tables(cfg)
    d_i0, d_w = mapping._gain_upload(i0, w)
    d_dct = evaluation._dct_device(cfg['n_mels'], n, 1)
    cy, cx = (cuda((0.05 * rng.standard_normal((Bm, Fm, n))).astype(np.float32)) for _ in range(2))
    tg = event_ms(lambda: mapping._gain_launch(cy, cx, lm, d_dct, d_i0, d_w, 1.0, 50.0, 20.0, 30.0), a.reps)
    gb = Bm * Fm * (201 + 2 * n) * 4
    say('vc_cep_gain_f32, %d x %d frames, 201 bins: %.4f / %.4f / %.4f ms; must move %.1f MB: %.1f %% of the HBM line'
        % (Bm, Fm, *tg, gb / 1e6, 100 * gb / HBM_BYTES_PER_S / (tg[0] * 1e-3)))
    # waveform in, waveform out at 16 x 5 s, against convert_diff_batch
    import ab_convert_batch as acb
    from bench import synth_audio
    dec, c = acb.models()
    L = 5 * c['sample_rate']
    wav = synth_audio(16, L, seed=300).float().cuda()
    m = mr.random_model(32, 48, seed=2, spread=0.5)
    model = mapping.JDGMM(*(cuda(m[k]) for k in mr.FIELDS))
    tw = wall_ms(lambda: conversion.convert_gmm_diff_batch(model, wav, None, c), a.reps)
    td = wall_ms(lambda: conversion.convert_diff_batch(dec, wav, None, c), a.reps)
    say('16 x 5 s, host clock to a device synchronise (median / min / max, ms): convert_gmm_diff_batch (M = 32, 24 cepstra) '
        '%.2f / %.2f / %.2f; convert_diff_batch (the decoder) %.2f / %.2f / %.2f' % (*tw, *td))
    # fit against the host
    xs, ys = mr.cepstral_corpus(n_utt=8, n=12, lo=150, hi=200)
    X, ln = mr.batch(xs)
    Y, _ = mr.batch(ys)
    hfa, hfb = mr.features_batch(X, ln), mr.features_batch(Y, ln)
    dfa, dfb = cuda(hfa), cuda(hfb)
    tf = wall_ms(lambda: mapping.fit(dfa, ln, dfb, ln, n_components=16, n_iter=10), max(a.reps // 3, 1))
    t0 = time.perf_counter()
    want, _ = mr.fit(hfa, hfb, ln, ln, n_components=16, n_iter=10)
    th = 1e3 * (time.perf_counter() - t0)
    got, _ = mapping.fit(dfa, ln, dfb, ln, n_components=16, n_iter=10)
    say('mapping.fit, 8 pairs of %d .. %d frames, D = 24, M = 16, 10 iterations: %.2f / %.2f / %.2f ms; tests/mapping_ref.py on the host '
        '(float64, one run) %.0f ms; largest difference of a mean %.2e' % (min(ln), max(ln), *tf, th,
                                                                          float(np.abs(got.mu_y.cpu().numpy() - want['mu_y']).max())))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
