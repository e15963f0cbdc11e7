"""Timing of phone-loop decoding (csrc/vc_decode.hip behind evaluation.decode_batch) on one MI355X: HIP events around the
calls, arms interleaved, medians.

Arms: evaluation.decode_batch on device tensors (kind='log': the two launches);
(a) tests/decode_ref.py, the float32 restatement in numpy, on the downloaded tensors (download included; wall clock --
    --ref-reps repetitions, it takes seconds);
(b) a torch formulation on the device: one step per frame over [B, C] tensors (the [B, C, C] sum and its maximum, the
    shift of the duration states, the moves kept), then a back-track of one step per frame;
(c) evaluation.phn_segments_batch on the same posteriors: the arg-max read-out the decoder replaces, so the ratio is the
    price of the better sequence.
Shapes: 16 and 256 utterances of about 1,000 frames, 61 classes, min_dur 1 and 3, speech-like log-posteriors
(tests/align_ref.py synthetic_posteriors, segments of 3 to 11 frames, noise 0.4), a bigram matrix with a -inf diagonal.
(b)'s path and the reference's outputs must equal the device's.

    python tools/ab_decode.py --reps 7 --out profiles/decode/ab_decode.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_decode.py --kernel-only --reps 5
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_decode.py --kernel-only --reps 5 --classes 128
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


def make_batch(B, seed):
    """(score [B, F_MAX, C], n_frames [B], trans [C, C]) from at most 8 distinct utterances."""
    import align_ref as ar
    import decode_ref as dr
    rng = np.random.RandomState(seed)
    base, seqs = [], []
    for k in range(min(B, 8)):
        F = int(rng.randint(F_MAX - 100, F_MAX + 1))
        labs, lens = [], []
        while sum(lens) < F:
            c = int(rng.randint(C))
            if not labs or c != labs[-1]:
                labs.append(c)
                lens.append(int(rng.randint(3, 12)))
        p = ar.synthetic_posteriors(labs, lens, C, seed=seed + k, peak=0.5, noise=0.4)[:F]
        score = np.zeros((F_MAX, C), np.float32)
        score[:F] = np.log(np.maximum(p, np.float32(1e-10)))
        base.append((score, F))
        seqs.append(labs[:100])
    pick = [base[b % len(base)] for b in range(B)]
    trans = dr.phn_transitions(np.array(seqs), np.full(len(seqs), 100), C)
    return np.stack([u[0] for u in pick]), np.array([u[1] for u in pick], np.int32), trans


def torch_decode(score, trans, n_frames, M):
    """Arm (b).  Returns frame_class [B, F] (-1 beyond n_frames; feasibility is not handled: the tool's data is feasible)."""
    import torch
    B, F, _ = score.shape
    dev = score.device
    D = torch.full((B, M, C), float('-inf'), device=dev)
    D[:, 0] = score[:, 0]
    bps = torch.zeros((F, B, C), dtype=torch.int64, device=dev)
    bits = torch.zeros((F, B, C), dtype=torch.bool, device=dev)
    for t in range(1, F):
        e = score[:, t]
        X, bp = (D[:, M - 1, :, None] + trans[None]).max(1)
        stay = D[:, M - 1]
        cand = X if M == 1 else D[:, M - 2]
        bit = cand > stay
        new = torch.empty_like(D)
        if M > 1:
            new[:, 0] = e + X
            new[:, 1:M - 1] = e[:, None] + D[:, 0:M - 2]
        new[:, M - 1] = e + torch.where(bit, cand, stay)
        D = torch.where((t < n_frames)[:, None, None], new, D)      # an utterance that has ended keeps its last rows
        bps[t], bits[t] = bp, bit
    c = D[:, M - 1].argmax(1)
    d = torch.full((B,), M - 1, dtype=torch.int64, device=dev)
    out = torch.full((B, F), -1, dtype=torch.int64, device=dev)
    for t in range(F - 1, -1, -1):
        on = t < n_frames
        out[:, t] = torch.where(on, c, out[:, t])
        bit = torch.gather(bits[t], 1, c[:, None])[:, 0]
        bp = torch.gather(bps[t], 1, c[:, None])[:, 0]
        if M == 1:
            enter, nd = bit, d
        else:
            enter = d == 0
            nd = torch.where(d == M - 1, torch.where(bit, M - 2, M - 1), d - 1)
            nd = torch.where(enter, M - 1, nd)
        upd = on & (t > 0)
        c, d = torch.where(upd & enter, bp, c), torch.where(upd, nd, d)
    return out.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--ref-reps', type=int, default=1)
    ap.add_argument('--kernel-only', action='store_true', help='the public call alone (for a kernel trace)')
    ap.add_argument('--classes', type=int, default=61, help='61: the one-wave forward kernel; above 64: the two-wave one')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    global C
    C = a.classes
    import torch
    import evaluation as ev
    import decode_ref as dr
    if not torch.cuda.is_available():
        raise SystemExit('ab_decode needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, M in ((16, 1), (16, 3), (256, 1), (256, 3)):
        h = make_batch(B, seed=100)
        score, nf, trans = (torch.from_numpy(v).cuda() for v in h)
        dev_call = lambda: ev.decode_batch(score, nf, trans=trans, min_dur=M, kind='log')

        def ref_call():
            t0 = time.perf_counter()
            got = dr.decode_batch_f32(score.cpu().numpy(), nf.cpu().numpy(), trans.cpu().numpy(), min_dur=M)
            return (time.perf_counter() - t0) * 1e3, got

        r = dev_call()
        torch.cuda.synchronize()
        say('%d utterances of %d .. %d frames, %d classes, min_dur %d: %.1f segments on average, workspace %.2f MB'
            % (B, int(nf.min()), int(nf.max()), C, M, float(r.seg.n_seg.float().mean()), B * C * ((F_MAX + 3) // 4) * 4 / 1e6))
        if a.kernel_only:
            for _ in range(a.reps):
                dev_call()
            torch.cuda.synchronize()
            continue
        tb = torch_decode(score, trans, nf, M)
        torch.cuda.synchronize()
        assert torch.equal(tb, r.frame_class), 'the torch formulation found another path'
        arms = {'decode_batch (device)': dev_call, '(b) torch, one step per frame': lambda: torch_decode(score, trans, nf, M),
                '(c) phn_segments_batch (arg-max)': lambda: ev.phn_segments_batch(score, nf, min_run=3)}
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k].append(timed(f))
        ref_ms = []
        for _ in range(a.ref_reps):
            ms, want = ref_call()
            ref_ms.append(ms)
        same = lambda x, y: np.array_equal(np.nan_to_num(x, nan=-1.0).view(np.uint32), np.nan_to_num(y, nan=-1.0).view(np.uint32))
        assert np.array_equal(want.frame_class, r.frame_class.cpu().numpy()) and same(want.total, r.total.cpu().numpy()) and \
            np.array_equal(want.seg_label, r.seg.labels.cpu().numpy()) and same(want.seg_score, r.seg_score.cpu().numpy()), \
            'the device differs from the reference'
        med = {}
        for k, v in times.items():
            med[k] = float(np.median(v))
            say('  %-34s median %10.3f ms  (min %.3f, max %.3f, %d reps)' % (k, med[k], min(v), max(v), len(v)))
        med_ref = float(np.median(ref_ms))
        say('  %-34s median %10.3f ms  (wall clock, download included, %d reps)' % ('(a) tests/decode_ref.py on the host', med_ref, len(ref_ms)))
        d = med['decode_batch (device)']
        say('  device against (a): %.0f x;  against (b): %.1f x;  against (c): %.2f x its time;  %.3f us per frame step of the batch'
            % (med_ref / d, med['(b) torch, one step per frame'] / d, d / med['(c) phn_segments_batch (arg-max)'], d * 1e3 / F_MAX))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
