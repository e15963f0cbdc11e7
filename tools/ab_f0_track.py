"""Timing of the pitch tracker with several candidates per frame (csrc/vc_f0.hip f0_candidates_kernel, csrc/vc_f0_track.hip)
on one MI355X: HIP events around the public calls, arms interleaved, medians.

Arms: evaluation.f0_batch (YIN, one decision per frame) against evaluation.f0_candidates_batch (the same d', then the
selection of up to n_cand local minima): the ratio is what the selection costs.  evaluation.f0_viterbi_batch on that
lattice: one wave per utterance, sequential over frames, so the figure is the time per frame step.  evaluation.
f0_track_batch: both launches.  Shapes: 16 x 5 s, 256 x 5 s, 1 x 60 s at 16 kHz.

    python tools/ab_f0_track.py --reps 9 --out profiles/f0_track/ab_f0_track.log
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

HOP = 80


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
    ap.add_argument('--n-cand', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import evaluation as ev
    import f0_track_ref as tr
    if not torch.cuda.is_available():
        raise SystemExit('ab_f0_track needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, seconds in ((16, 5.0), (256, 5.0), (1, 60.0)):
        base = [tr.weak_signal(30 + k, seconds=seconds)[0] for k in range(min(B, 4))]
        wav = torch.from_numpy(np.stack([base[k % len(base)] for k in range(B)])).cuda()
        L = wav.shape[1]
        lens = [L] * B
        c = ev.f0_candidates_batch(wav, lens, n_cand=a.n_cand)
        arms = {'f0_batch (YIN)': lambda: ev.f0_batch(wav, lens),
                'f0_candidates_batch': lambda: ev.f0_candidates_batch(wav, lens, n_cand=a.n_cand),
                'f0_viterbi_batch': lambda: ev.f0_viterbi_batch(c.pitch, c.cost, c.n, c.frames, f0=c.f0),
                'f0_track_batch': lambda: ev.f0_track_batch(wav, lens, n_cand=a.n_cand)}
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k].append(timed(f))
        F = 1 + L // HOP
        say('%d utterances of %.0f s (%d frames each), n_cand %d, %.2f candidates per frame:'
            % (B, seconds, F, a.n_cand, float(c.n.float().mean())))
        med = {}
        for k, v in times.items():
            med[k] = float(np.median(v))
            say('  %-20s median %9.3f ms  (min %.3f, max %.3f, %d reps)' % (k, med[k], min(v), max(v), len(v)))
        say('  candidates / YIN: %.3f;  Viterbi: %.3f us per frame step of one utterance (%d steps in sequence, launch and '
            'upload of the lengths included)' % (med['f0_candidates_batch'] / med['f0_batch (YIN)'], med['f0_viterbi_batch'] * 1e3 / F, F))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
