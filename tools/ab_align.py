"""Timing of forced alignment (csrc/vc_align.hip behind evaluation.align_batch) on one MI355X: HIP events around the calls,
arms interleaved, medians.

Arms: evaluation.align_batch on device tensors (kind='log': the two launches and labels = seq[frame_state]);
(a) tests/align_ref.py, the float32 restatement in numpy, on the downloaded tensors (download included; wall clock --
    --ref-reps repetitions, it takes seconds);
(b) a torch formulation on the device: the emissions gathered once, then one step per frame over [B, S] tensors (shifted
    copies, two compare-selects, one add, the codes kept), then a back-track of one step per frame.
Shapes: 16 and 256 utterances of about 1,000 frames by 60 and by 300 states, 61 classes, speech-like log-posteriors
(tests/align_ref.py synthetic_posteriors), one state in six optional.  (b)'s path must equal the device's.

    python tools/ab_align.py --reps 7 --out profiles/align/ab_align.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_align.py --kernel-only --reps 5
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

C = 61
F_MAX = 1000


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def make_batch(B, S, seed):
    """(score [B, F_MAX, C], seq [B, S], opt [B, S], n_frames [B], n_seq [B]) from at most 8 distinct utterances."""
    import align_ref as ar
    rng = np.random.RandomState(seed)
    base = []
    for k in range(min(B, 8)):
        F = int(rng.randint(F_MAX - 100, F_MAX + 1))
        seq = rng.randint(0, C, size=S)
        opt = (np.arange(S) % 6 == 5).astype(np.uint8)
        present = np.ones(S, bool)
        present[opt.astype(bool) & (rng.rand(S) < 0.5)] = False       # half of the optional states are not in the audio
        n = int(present.sum())
        cuts = np.sort(rng.choice(np.arange(1, F), size=n - 1, replace=False))
        lens = np.diff(np.concatenate([[0], cuts, [F]]))
        p = ar.synthetic_posteriors(seq[present], lens, C, seed=seed + k)
        score = np.zeros((F_MAX, C), np.float32)
        score[:F] = np.log(np.maximum(p, np.float32(1e-10)))
        base.append((score, seq.astype(np.int32), opt, F))
    pick = [base[b % len(base)] for b in range(B)]
    return (np.stack([u[0] for u in pick]), np.stack([u[1] for u in pick]), np.stack([u[2] for u in pick]),
            np.array([u[3] for u in pick], np.int32), np.full((B,), S, np.int32))


def torch_align(score, seq, opt, n_frames, n_seq):
    """Arm (b).  Returns frame_state [B, F] (-1 beyond n_frames; feasibility is not handled: the tool's data is feasible)."""
    import torch
    B, F, _ = score.shape
    S = seq.shape[1]
    dev = score.device
    ninf = torch.tensor(float('-inf'), device=dev)
    e = torch.gather(score, 2, seq.long()[:, None, :].expand(B, F, S))
    sidx = torch.arange(S, device=dev)[None, :]
    live = sidx < n_seq[:, None]
    e = torch.where(live[:, None, :], e, ninf)
    skip = torch.zeros((B, S), dtype=torch.bool, device=dev)
    skip[:, 2:] = opt[:, 1:S - 1] != 0
    first = (sidx == 0) | ((sidx == 1) & (opt[:, :1] != 0))
    d = torch.where(first, e[:, 0], ninf)
    codes = torch.zeros((F, B, S), dtype=torch.int64, device=dev)
    pad = ninf.expand(B, 2)
    for t in range(1, F):
        p1 = torch.cat([pad[:, :1], d[:, :-1]], 1)
        p2 = torch.cat([pad, d[:, :-2]], 1)
        a = p1 > d
        best = torch.where(a, p1, d)
        k = skip & (p2 > best)
        best = torch.where(k, p2, best)
        codes[t] = a.long() * (~k).long() + 2 * k.long()
        nd = e[:, t] + best
        run = (t < n_frames)[:, None]
        d = torch.where(run, nd, d)                                 # an utterance that has ended keeps its last row
    last = d
    fin = (n_seq - 1).long()
    prev = (fin - 1).clamp_min(0)
    take_prev = (n_seq >= 2) & (torch.gather(opt, 1, fin[:, None])[:, 0] != 0) & \
        (torch.gather(last, 1, prev[:, None])[:, 0] > torch.gather(last, 1, fin[:, None])[:, 0])
    s = torch.where(take_prev, prev, fin)
    out = torch.full((B, F), -1, dtype=torch.int64, device=dev)
    for t in range(F - 1, -1, -1):
        on = t < n_frames
        out[:, t] = torch.where(on, s, out[:, t])
        c = torch.gather(codes[t], 1, s[:, None])[:, 0]
        s = torch.where(on, s - c, s)
    return out.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--ref-reps', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true', help='the public call alone (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import evaluation as ev
    import align_ref as ar
    if not torch.cuda.is_available():
        raise SystemExit('ab_align needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, S in ((16, 60), (16, 300), (256, 60), (256, 300)):
        h = make_batch(B, S, seed=100 + S)
        score, seq, opt, nf, ns = (torch.from_numpy(v).cuda() for v in h)
        dev_call = lambda: ev.align_batch(score, nf, seq, ns, optional=opt, kind='log')

        def ref_call():
            t0 = time.perf_counter()
            got = ar.align_batch_f32(*(v.cpu().numpy() for v in (score, seq, opt, nf, ns)))
            return (time.perf_counter() - t0) * 1e3, got

        r = dev_call()
        torch.cuda.synchronize()
        words = (F_MAX + 15) // 16
        say('%d utterances of %d .. %d frames x %d states (%d classes): K = %d states per lane, %d visited on average, workspace %.2f MB'
            % (B, int(nf.min()), int(nf.max()), S, C, next(k for k in (1, 2, 4, 8, 16) if 64 * k >= S), float(r.n_visited.float().mean()),
               B * words * S * 4 / 1e6))
        if a.kernel_only:
            for _ in range(a.reps):
                dev_call()
            torch.cuda.synchronize()
            continue
        tb = torch_align(score, seq, opt, nf, ns)
        torch.cuda.synchronize()
        assert torch.equal(tb, r.frame_state), 'the torch formulation found another path'
        arms = {'align_batch (device)': dev_call, '(b) torch, one step per frame': lambda: torch_align(score, seq, opt, nf, ns)}
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k].append(timed(f))
        ref_ms = []
        for _ in range(a.ref_reps):
            ms, want = ref_call()
            ref_ms.append(ms)
        assert np.array_equal(want.frame_state, r.frame_state.cpu().numpy()) and \
            np.array_equal(want.total.view(np.uint32), r.total.cpu().numpy().view(np.uint32)), 'the device differs from the reference'
        med = {}
        for k, v in times.items():
            med[k] = float(np.median(v))
            say('  %-32s median %10.3f ms  (min %.3f, max %.3f, %d reps)' % (k, med[k], min(v), max(v), len(v)))
        med_ref = float(np.median(ref_ms))
        say('  %-32s median %10.3f ms  (wall clock, download included, %d reps)' % ('(a) tests/align_ref.py on the host', med_ref, len(ref_ms)))
        d = med['align_batch (device)']
        say('  device against (a): %.0f x;  against (b): %.1f x;  %.3f us per frame step of the batch, %.2f ns per cell'
            % (med_ref / d, med['(b) torch, one step per frame'] / d, d * 1e3 / F_MAX, d * 1e6 / (float(nf.sum()) * S)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
