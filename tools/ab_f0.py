"""A/B of the YIN F0 kernel (csrc/vc_f0.hip) on one MI355X: HIP events around the public call, arms interleaved, medians.

Arms: the kernel (evaluation.f0_batch); a torch form on the same device that a user would write today (unfold into
frames, the differences as energy terms minus an FFT cross-correlation, cumulative sum, first-below-threshold by argmax;
float32, so it carries the cancellation the direct form avoids); the float64 host reference of tests/f0_ref.py for one
utterance, extrapolated to the batch.  Shapes: 16 x 5 s, 256 x 5 s, 1 x 60 s at 16 kHz.

    python tools/ab_f0.py --reps 9 --out profiles/f0/ab_f0.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_f0.py --kernel-only --reps 5
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d OUT -- python tools/ab_f0.py --kernel-only --reps 2
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

HOP, W, TAU_MIN, TAU_MAX, THR, SR = 80, 512, 40, 267, 0.15, 16000.0


def torch_yin(wav, chunk=1024):
    """wav [B, L] float32 on the device, equal lengths -> f0 [B, F].  Frames in chunks to bound the unfolded copy."""
    import torch
    B, L = wav.shape
    span, half = W + TAU_MAX + 1, (W + TAU_MAX) // 2
    F = 1 + L // HOP
    x = torch.nn.functional.pad(wav, (half, span + HOP))
    fr_all = x.unfold(1, span, HOP)[:, :F]                                     # a view
    n_lag = TAU_MAX + 2
    nfft = 2048
    out = []
    lag = torch.arange(n_lag, device=wav.device, dtype=torch.float32)
    for f0 in range(0, F, chunk):
        fr = fr_all[:, f0:f0 + chunk]
        a = fr[..., :W]
        corr = torch.fft.irfft(torch.fft.rfft(a, nfft).conj() * torch.fft.rfft(fr, nfft), nfft)[..., :n_lag]   # sum_j a[j] fr[j + tau]
        sq = torch.cumsum(torch.nn.functional.pad(fr * fr, (1, 0)), -1)
        e0 = sq[..., W:W + 1] - sq[..., 0:1]
        et = sq[..., W:W + n_lag] - sq[..., 0:n_lag]
        d = (e0 + et - 2.0 * corr).clamp_min(0.0)
        d[..., 0] = 0.0
        S = torch.cumsum(d, -1)
        dp = torch.where(S > 0, d * lag / S, torch.ones_like(d))
        dp[..., 0] = 1.0
        rng = dp[..., TAU_MIN:TAU_MAX + 1]
        below = rng < THR
        first = torch.argmax(below.to(torch.int8), -1)
        # walk to the bottom of the dip: the first lag from `first` on whose successor is not smaller
        rise = torch.nn.functional.pad(rng[..., 1:] >= rng[..., :-1], (0, 1), value=True)
        idx = torch.arange(rng.shape[-1], device=wav.device)
        stop = torch.where(rise & (idx >= first[..., None]), idx, torch.full_like(idx, rng.shape[-1])).amin(-1)
        tau = stop + TAU_MIN
        y = torch.gather(dp, -1, torch.stack([tau - 1, tau, tau + 1], -1))
        den = y[..., 0] - 2.0 * y[..., 1] + y[..., 2]
        off = torch.where(den > 0, 0.5 * (y[..., 0] - y[..., 2]) / den, torch.zeros_like(den)).clamp(-0.5, 0.5)
        out.append(torch.where(below.any(-1), SR / (tau.float() + off), torch.zeros_like(off)))
    return torch.cat(out, 1)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--kernel-only', action='store_true', help='only the kernel arm, no events: for a kernel trace')
    a = ap.parse_args()
    import torch
    import evaluation as ev
    import f0_ref as fr
    if not torch.cuda.is_available():
        raise SystemExit('ab_f0 needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, seconds in ((16, 5.0), (256, 5.0), (1, 60.0)):
        base = [fr.glide_signal(30 + k, seconds=seconds)[0] for k in range(min(B, 4))]
        wav = torch.from_numpy(np.stack([base[k % len(base)] for k in range(B)])).cuda()
        L = wav.shape[1]
        lens = [L] * B
        arms = {'kernel': lambda: ev.f0_batch(wav, lens)}
        if a.kernel_only:
            for _ in range(a.reps):
                arms['kernel']()
            torch.cuda.synchronize()
            continue
        arms['torch unfold + FFT'] = lambda: torch_yin(wav)
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k].append(timed(f))
        F = 1 + L // HOP
        terms = B * F * (TAU_MAX + 2) * W
        say('%d utterances of %.0f s (%d frames each, %.3g terms):' % (B, seconds, F, terms))
        for k, v in times.items():
            med = float(np.median(v))
            say('  %-20s median %9.3f ms  (min %.3f, max %.3f, %d reps)  %.1f Gterm/s' % (k, med, min(v), max(v), len(v), terms / med / 1e6))
        got, other = ev.f0_batch(wav, lens).f0[:4].cpu().numpy(), torch_yin(wav)[:4].cpu().numpy()
        vv = (got > 0) & (other > 0)
        say('  kernel vs torch form: voicing differs on %d of %d frames; on frames voiced in both, max |difference| %.3f cents, median %.2e'
            % (int(((got > 0) != (other > 0)).sum()), got.size, np.abs(fr.cents(got[vv], other[vv])).max(), np.median(np.abs(fr.cents(got[vv], other[vv])))))
        if not a.skip_host and B == 16:
            t0 = time.perf_counter()
            want, _ = fr.yin(wav[0].cpu().numpy())
            dt = time.perf_counter() - t0
            vv = (got[0] > 0) & (want > 0)
            say('  host float64 reference, one utterance incl. copy down: %.0f ms (x %d = %.1f s); device max |difference| %.2e cents'
                % (dt * 1e3, B, dt * B, np.abs(fr.cents(got[0][vv], want[vv])).max()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
