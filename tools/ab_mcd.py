"""A/B of the DTW scoring kernel (csrc/vc_dtw.hip) on one MI355X: HIP events around the call, arms interleaved, medians.

Arms: the kernel in score mode and in path mode (back-track included); (b) a torch form on the same device that updates
one anti-diagonal per step (the frame distances as one batched matrix product up front, which the kernel never stores);
(a) the float64 host reference of tests/mcd_ref.py including the copy down (one pair, extrapolated to the batch: it is
three orders of magnitude away).  Shapes: 16 and 256 pairs of 5 s (1,001 x 1,100 frames), one pair of 60 s.

    python tools/ab_mcd.py --reps 9 --out profiles/mcd/ab_mcd.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_mcd.py --kernel-only --reps 5
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def torch_antidiagonal(ca, cb, scale):
    """[B, Fa, C] x [B, Fb, C], equal lengths in the batch: total [B].  Skewed storage: row i of the distance matrix is
    shifted right by i, so an anti-diagonal is a column."""
    import torch
    B, Fa, _ = ca.shape
    Fb = cb.shape[1]
    d2 = (ca * ca).sum(-1)[:, :, None] + (cb * cb).sum(-1)[:, None, :] - 2.0 * torch.bmm(ca, cb.transpose(1, 2))
    d = scale * torch.sqrt(2.0 * d2.clamp_min(0.0))
    inf = float('inf')
    sk = torch.full((B, Fa, Fa + Fb - 1), inf, device=ca.device)
    idx = torch.arange(Fb, device=ca.device)[None, :] + torch.arange(Fa, device=ca.device)[:, None]
    sk.scatter_(2, idx[None].expand(B, -1, -1), d)
    D2 = torch.full((B, Fa + 1), inf, device=ca.device)
    D1 = torch.full((B, Fa + 1), inf, device=ca.device)
    D2[:, 0] = 0.0
    for k in range(Fa + Fb - 1):
        best = torch.minimum(torch.minimum(D2[:, :-1], D1[:, :-1]), D1[:, 1:])
        Dk = torch.full_like(D1, inf)
        Dk[:, 1:] = sk[:, :, k] + best
        D2, D1 = D1, Dk
    return D1[:, Fa]


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--kernel-only', action='store_true', help='only the kernel arms, no events: for a kernel trace')
    a = ap.parse_args()
    import torch
    import evaluation as ev
    import mcd_ref as mr
    if not torch.cuda.is_available():
        raise SystemExit('ab_mcd needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    for B, Fa, Fb, with_torch in ((16, 1001, 1100, True), (256, 1001, 1100, True), (1, 12000, 12000, False)):
        # smooth random cepstra (a random walk over frames), the same statistics on both sides
        ca = torch.from_numpy(np.cumsum(rng.standard_normal((B, Fa, 24)).astype(np.float32) * 0.05, axis=1)).cuda()
        cb = torch.from_numpy(np.cumsum(rng.standard_normal((B, Fb, 24)).astype(np.float32) * 0.05, axis=1)).cuda()
        la, lb = [Fa] * B, [Fb] * B
        arms = {'kernel score': lambda: ev.dtw_batch(ca, cb, la, lb, scale=25.0),
                'kernel path': lambda: ev.dtw_batch(ca, cb, la, lb, scale=25.0, return_path=True)}
        if a.kernel_only:
            for _ in range(a.reps):
                for f in arms.values():
                    f()
            torch.cuda.synchronize()
            continue
        if with_torch:
            arms['torch anti-diagonal'] = lambda: torch_antidiagonal(ca, cb, 25.0)
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k] += timed(f, 1)
        cells = B * Fa * Fb
        say('%d pairs of %d x %d frames (%.3g cells, %d serial steps per pass):' % (B, Fa, Fb, cells, Fb + 255))
        for k, v in times.items():
            med = float(np.median(v))
            say('  %-22s median %10.3f ms  (min %.3f, max %.3f, %d reps)  %.2f Gcell/s' % (k, med, min(v), max(v), len(v), cells / med / 1e6))
        if with_torch:
            got, want = ev.dtw_batch(ca, cb, la, lb, scale=25.0).total, torch_antidiagonal(ca, cb, 25.0)
            say('  kernel vs torch form: max rel diff of totals %.2e' % float(((got - want).abs() / want).max()))
        if not a.skip_host and B == 16:
            t0 = time.perf_counter()
            x, y = ca[0].cpu().numpy(), cb[0].cpu().numpy()
            t64 = mr.dtw(x, y, 25.0, want_path=False)[0]
            dt = time.perf_counter() - t0
            say('  host float64 reference, one pair incl. copy down: %.0f ms (x %d pairs = %.1f s); device total rel diff %.2e'
                % (dt * 1e3, B, dt * B, abs(float(ev.dtw_batch(ca[:1], cb[:1], [Fa], [Fb], scale=25.0).total[0]) - t64) / t64))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
