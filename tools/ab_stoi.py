"""Timing of the intelligibility scores (csrc/vc_stoi.hip behind evaluation.stoi_batch and si_sdr_batch) on one MI355X: HIP
events, arms interleaved, medians.

At 16 x 5 s and at 256 x 5 s of synthetic speech at 10 kHz with white noise at 10 dB:
  a float4 copy of the two waveforms' bytes (torch's copy_), the yardstick; each launch alone on the device's own inputs
  (vc_stoi_energy_f32, vc_stoi_keep_f32, vc_stoi_bands_f32, vc_stoi_score_f32 in both modes, vc_si_sdr_f32); stoi_batch
  whole.  Event figures include the launch gap of a call from Python; stoi_batch's also the allocation of its outputs.
  Then the float64 numpy restatement (tests/stoi_ref.py) of the same batch on the host, wall clock, once.
With --vowel: STOI / ESTOI / SI-SDR of the synthetic noisy vowel of tests/denoise_ref.py (16 kHz, resampled by stoi_batch)
before and after enhance.denoise_batch at 0 / 10 / 20 dB: a report, not a claim.

    python tools/ab_stoi.py --reps 7 --vowel --out profiles/stoi/ab_stoi.log
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_warp import interleaved                                     # noqa: E402  (the same timing loops)

L = 50000                                                           # 5 s at 10 kHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50, help='back-to-back launches per kernel timing')
    ap.add_argument('--host-utts', type=int, default=16, help='utterances the numpy restatement is timed on')
    ap.add_argument('--vowel', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import _vc
    import evaluation as ev
    import stoi_ref as sr
    if not torch.cuda.is_available():
        raise SystemExit('ab_stoi needs a GPU')
    from bench import synth_audio
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(t):
        for k, v in t.items():
            say('  %-60s median %9.4f ms  (min %.4f, max %.4f, %d reps)' % (k, float(np.median(v)), min(v), max(v), len(v)))

    lib = _vc.lib()
    ratio = float(np.float32(1e-4))
    for B in (16, 256):
        clean = synth_audio(B, L, seed=300)
        g = torch.Generator().manual_seed(5)
        noise = torch.randn(clean.shape, generator=g) * float(clean.pow(2).mean().sqrt()) * 10.0 ** (-10.0 / 20.0)
        ref, deg = clean.cuda().contiguous(), (clean + noise).cuda().contiguous()
        d_len = torch.full((B,), L, dtype=torch.int32, device='cuda')
        Fmax = ev.stoi_frames(L)
        Mmax, Smax = Fmax - 1, Fmax - ev.STOI_SEG
        tab = ev._stoi_bands_device()
        nb = int(tab.shape[0])
        dev = ref.device
        e, nf = torch.empty((B, Fmax), device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        idx, K = torch.empty((B, Fmax), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        T = torch.empty((2, B, Mmax, nb), device=dev)
        seg, score, ns = torch.empty((B, Smax), device=dev), torch.empty((B,), device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        sd, va = torch.empty((B,), device=dev), torch.empty((B,), dtype=torch.uint8, device=dev)
        both, dst = torch.stack([ref, deg]), torch.empty((2, B, L), device=dev)
        st = _vc.current_stream()
        P = _vc.ptr

        def energy():
            _vc.check(lib.vc_stoi_energy_f32(P(ref), P(d_len), B, L, L, P(e), P(nf), Fmax, st))

        def keep():
            _vc.check(lib.vc_stoi_keep_f32(P(e), P(nf), B, Fmax, ratio, P(idx), P(K), st))

        def bands():
            _vc.check(lib.vc_stoi_bands_f32(P(ref), P(deg), B, L, L, P(idx), P(K), Fmax, P(tab), nb, P(T), Mmax, st))

        def scores(mode):
            _vc.check(lib.vc_stoi_score_f32(P(T), P(K), B, Fmax, Mmax, nb, mode, P(seg), Smax, P(score), P(ns), st))

        def sdr():
            _vc.check(lib.vc_si_sdr_f32(P(ref), P(deg), P(d_len), B, L, L, 1, P(sd), P(va), st))

        energy(), keep(), bands(), scores(0)
        torch.cuda.synchronize()
        say('%d x %d samples at 10 kHz, white noise 10 dB under the synthetic speech: %d frames, %d kept on average, STOI %.3f'
            % (B, L, Fmax, float(K.float().mean()), float(score.mean())))
        arms = {'float4 copy of both waveforms (torch copy_, %.1f MB)' % (both.numel() * 4 / 1e6): lambda: dst.copy_(both),
                'vc_stoi_energy_f32': energy, 'vc_stoi_keep_f32': keep, 'vc_stoi_bands_f32': bands,
                'vc_stoi_score_f32, STOI (two launches)': lambda: scores(0), 'vc_stoi_score_f32, ESTOI (two launches)': lambda: scores(1),
                'vc_si_sdr_f32': sdr,
                'stoi_batch, every launch': lambda: ev._stoi_launch(ref, deg, d_len, 0, ratio, False)}
        say('launches (HIP events over %d back-to-back calls, launch gaps included)' % a.inner)
        report(interleaved(arms, a.reps, a.inner))
        n = min(a.host_utts, B)
        scores(0)                                                   # (the ESTOI arm ran last)
        torch.cuda.synchronize()
        x, y =ref[:n].cpu().numpy().astype(np.float64), deg[:n].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        host = [sr.stoi(x[b], y[b]) for b in range(n)]
        dt = time.perf_counter() - t0
        say('  float64 numpy restatement on the host: %.1f ms for %d utterances (%.1f ms each; largest |device - host| %.2e)'
            % (1e3 * dt, n, 1e3 * dt / n, float(np.abs(score[:n].cpu().numpy() - np.array(host)).max())))

    if a.vowel:
        import denoise_ref as dr
        import enhance
        say('the noisy vowel of tests/denoise_ref.py (120 Hz, 16 kHz, 0.6 s of noise alone first), scored against the clean vowel '
            'before and after enhance.denoise_batch; stoi_batch resamples both sides to 10 kHz')
        for snr in (0, 10, 20):
            clean, noise = dr.noisy_vowel(120.0, snr, seed=130 + snr)
            x = clean.astype(np.float32)[None]
            noisy = (clean + noise).astype(np.float32)[None]
            y = enhance.denoise_batch(noisy, [noisy.shape[1]]).y
            n = int(y.shape[1])                                     # hop (F - 1) samples come back
            row = []
            for name, d in (('noisy', torch.from_numpy(noisy[:, :n]).cuda()), ('denoised', y)):
                r = torch.from_numpy(x[:, :n]).cuda()
                s = ev.stoi_batch(r, d, None, wav_sr=16000)
                e2 = ev.stoi_batch(r, d, None, wav_sr=16000, extended=True)
                q = ev.si_sdr_batch(r, d)
                row.append('%s STOI %.3f ESTOI %.3f SI-SDR %6.2f dB' % (name, float(s.score[0]), float(e2.score[0]), float(q.si_sdr[0])))
            say('  %2d dB: %s (%d segments)' % (snr, '; '.join(row), int(s.n_segments[0])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
