"""A/B of the speech-activity launches (csrc/vc_activity.hip) on one MI355X: HIP events around the public call, arms
interleaved, medians.

Arms: evaluation.activity_batch against a plain torch form of the same definition (unfold, square, sum, the gap fill from
cummax scans of the previous / next active frame, cumsum for the positions); masked score_wav_batch against unmasked
score_wav_batch on the same tree.  The third comparison, unmasked score_wav_batch on this tree against the parent
commit, is two runs of ``--unmasked-only`` in the two checkouts: nothing in that path changed, so the two medians must
sit inside the run-to-run spread.  Shapes: 16 x 5 s, 256 x 5 s, 1 x 60 s at 16 kHz, a third of every utterance silent.

    python tools/ab_activity.py --reps 9 --out profiles/activity/ab_activity.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_activity.py --kernel-only --reps 5
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

HOP, W, MAX_GAP = 80, 400, 20


def torch_activity(wav, ratio=1e-4):
    """wav [B, L] float32 on the device, equal lengths -> (mask [B, F] bool, index [B, F] int64, n_active [B])."""
    import torch
    B, L = wav.shape
    F = 1 + L // HOP
    x = torch.nn.functional.pad(wav, (W // 2, W + HOP))
    e = x.unfold(1, W, HOP)[:, :F].square().sum(-1)
    raw = (e > 0) & (e > ratio * e.amax(1, keepdim=True))
    pos = torch.arange(F, device=wav.device).expand(B, F)
    prev = torch.cummax(torch.where(raw, pos, torch.full_like(pos, -1)), 1).values
    nxt = torch.flip(torch.cummin(torch.flip(torch.where(raw, pos, torch.full_like(pos, F)), [1]), 1).values, [1])
    mask = raw | ((prev >= 0) & (nxt < F) & (nxt - prev - 1 <= MAX_GAP))
    k = torch.cumsum(mask.long(), 1) - 1
    index = torch.full((B, F + 1), -1, dtype=torch.long, device=wav.device)
    index.scatter_(1, torch.where(mask, k, torch.full_like(k, F)), pos)
    return mask, index[:, :F], mask.sum(1)


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
    ap.add_argument('--kernel-only', action='store_true', help='only the kernel arms, no events: for a kernel trace')
    ap.add_argument('--unmasked-only', action='store_true', help='only unmasked score_wav_batch: run in two checkouts to compare them')
    a = ap.parse_args()
    import torch
    import evaluation as ev
    import f0_ref as fr
    if not torch.cuda.is_available():
        raise SystemExit('ab_activity needs a GPU')
    cfg = json.load(open(os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'ds_cfg_d.json'))) if os.path.exists(
        os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'ds_cfg_d.json')) else __import__('test_mcd_cpu').CFG
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, seconds in ((16, 5.0), (256, 5.0), (1, 60.0)):
        base = [fr.glide_signal(40 + k, seconds=seconds)[0] for k in range(min(B, 4))]
        for x in base:                                                   # a third of every utterance is noise floor
            n = len(x)
            x[2 * n // 3:] = 3e-4 * np.random.RandomState(n).standard_normal(n - 2 * n // 3)
        wav = torch.from_numpy(np.stack([base[k % len(base)] for k in range(B)])).cuda()
        other = torch.roll(wav, 1, 0) if B > 1 else torch.flip(wav, [1]).contiguous()
        lens = [wav.shape[1]] * B
        arms = {}
        if not a.unmasked_only:
            arms['activity_batch'] = lambda: ev.activity_batch(wav, lens)
            arms['score_wav_batch masked'] = lambda: ev.score_wav_batch(wav, lens, other, lens, cfg, mask='energy')
        arms['score_wav_batch unmasked'] = lambda: ev.score_wav_batch(wav, lens, other, lens, cfg)
        if a.kernel_only:
            for _ in range(a.reps):
                for f in arms.values():
                    f()
            torch.cuda.synchronize()
            continue
        if not a.unmasked_only:
            arms['torch unfold + scans'] = lambda: torch_activity(wav)
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k].append(timed(f))
        say('%d utterances of %.0f s (%d frames each):' % (B, seconds, 1 + wav.shape[1] // HOP))
        for k, v in times.items():
            say('  %-26s median %9.3f ms  (min %.3f, max %.3f, %d reps)' % (k, float(np.median(v)), min(v), max(v), len(v)))
        if not a.unmasked_only:
            r, t = ev.activity_batch(wav, lens), torch_activity(wav)
            say('  kernel vs torch form: the mask differs on %d of %d frames; active %d of %d frames of the first utterance'
                % (int((r.mask.bool() != t[0]).sum()), t[0].numel(), int(r.n_active[0]), t[0].shape[1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
