"""Timing of full-sum alignment (csrc/vc_fullsum.hip behind evaluation.align_posterior_batch) on one MI355X: HIP events
around the calls, arms interleaved, medians.

Arms: evaluation.align_posterior_batch on device tensors (kind='log', no state posteriors: the two launches);
(a) evaluation.align_batch on the same tensors: the same lattice and geometry, one add and two compare-selects per cell
    where the full sum takes two lse of three terms, no stored row and no second pass over the frames;
(b) a torch formulation on the device: the emissions gathered once, then one logsumexp step per frame over [B, S] tensors,
    each row shifted by its maximum, forward with the rows kept and backward with gamma = softmax(alpha + beta) per frame;
    its gamma is checked against the device's;
(c) tests/fullsum_ref.py, the float64 restatement in numpy, on the downloaded tensors of at most --ref-utts utterances
    (wall clock, download included; the figure for the whole batch is that time scaled by the utterance count and is
    printed as such).
Shapes: those of tools/ab_align.py -- 16 and 256 utterances of about 1,000 frames by 60 and by 300 states, 61 classes,
speech-like log-posteriors, one state in six optional.

    python tools/ab_fullsum.py --reps 7 --out profiles/fullsum/ab_fullsum.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_fullsum.py --kernel-only --reps 5
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

from ab_align import C, F_MAX, make_batch, timed        # noqa: E402  (the shapes and the data of the forced-alignment tool)


def torch_fullsum(score, seq, opt, n_frames, n_seq):
    """Arm (b).  Returns (gamma [B, F, S], zero beyond n_frames; log_z [B]).  Feasibility is not handled: the tool's data is
    feasible."""
    import torch
    B, F, _ = score.shape
    S = seq.shape[1]
    dev = score.device
    ninf = torch.tensor(float('-inf'), device=dev)
    e = torch.gather(score, 2, seq.long()[:, None, :].expand(B, F, S))
    sidx = torch.arange(S, device=dev)[None, :]
    e = torch.where((sidx < n_seq[:, None])[:, None, :], e, ninf)
    skip_in = torch.zeros((B, S), dtype=torch.bool, device=dev)
    skip_in[:, 2:] = opt[:, 1:S - 1] != 0
    skip_out = torch.zeros((B, S), dtype=torch.bool, device=dev)
    skip_out[:, :S - 2] = (opt[:, 1:S - 1] != 0) & (sidx[:, 2:] < n_seq[:, None])
    first = (sidx == 0) | ((sidx == 1) & (opt[:, :1] != 0))
    fin = (n_seq - 1).long()[:, None]
    last = (sidx == fin) | ((sidx == fin - 1) & (torch.gather(opt, 1, fin) != 0))
    pad = ninf.expand(B, 2)
    alpha = torch.empty((F, B, S), dtype=torch.float32, device=dev)
    a = torch.where(first, e[:, 0], ninf)
    shift = torch.zeros((B,), dtype=torch.float64, device=dev)
    for t in range(F):
        if t:
            p1 = torch.cat([pad[:, :1], a[:, :-1]], 1)
            p2 = torch.where(skip_in, torch.cat([pad, a[:, :-2]], 1), ninf)
            a = torch.where((t < n_frames)[:, None], e[:, t] + torch.logsumexp(torch.stack([a, p1, p2]), 0), a)
        m = a.max(1).values
        a = a - m[:, None]
        shift += torch.where(t < n_frames, m, torch.zeros_like(m)).double()
        alpha[t] = a
    log_z = (shift + torch.logsumexp(torch.where(last, a, ninf), 1).double()).float()
    gamma = torch.zeros((B, F, S), dtype=torch.float32, device=dev)
    b = torch.where(last, torch.zeros_like(a), ninf)
    for t in range(F - 1, -1, -1):
        if t < F - 1:
            g = b + e[:, t + 1]
            n1 = torch.cat([g[:, 1:], pad[:, :1]], 1)
            n2 = torch.where(skip_out, torch.cat([g[:, 2:], pad], 1), ninf)
            nb = torch.logsumexp(torch.stack([g, n1, n2]), 0)
            nb = nb - nb.max(1).values[:, None]
            b = torch.where((t < n_frames - 1)[:, None], nb, b)      # an utterance that has not begun keeps its end row
        gamma[:, t] = torch.where((t < n_frames)[:, None], torch.softmax(alpha[t] + b, 1), gamma[:, t])
    return gamma, log_z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--ref-utts', type=int, default=8, help='utterances the host reference is timed on')
    ap.add_argument('--kernel-only', action='store_true', help='the public call alone (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import evaluation as ev
    import fullsum_ref as fr
    if not torch.cuda.is_available():
        raise SystemExit('ab_fullsum needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, S in ((16, 60), (16, 300), (256, 60), (256, 300)):
        h = make_batch(B, S, seed=100 + S)
        score, seq, opt, nf, ns = (torch.from_numpy(v).cuda() for v in h)
        dev_call = lambda: ev.align_posterior_batch(score, nf, seq, ns, optional=opt, kind='log')
        r = ev.align_posterior_batch(score, nf, seq, ns, optional=opt, kind='log', return_states=True)
        torch.cuda.synchronize()
        assert bool(r.feasible.all())
        say('%d utterances of %d .. %d frames x %d states (%d classes): K = %d states per lane, workspace %.2f MB, log Z %.1f .. %.1f'
            % (B, int(nf.min()), int(nf.max()), S, C, next(k for k in (1, 2, 4, 8, 16) if 64 * k >= S), B * F_MAX * S * 4 / 1e6,
               float(r.log_z.min()), float(r.log_z.max())))
        if a.kernel_only:
            for _ in range(a.reps):
                dev_call()
            torch.cuda.synchronize()
            continue
        tg, tz = torch_fullsum(score, seq, opt, nf, ns)
        torch.cuda.synchronize()
        d_gamma, d_lz = float((tg - r.state_post).abs().max()), float((tz - r.log_z).abs().max())
        assert d_gamma < 1e-3 and d_lz < 0.05, ('the torch formulation differs from the device', d_gamma, d_lz)
        n_ref = min(B, a.ref_utts)
        t0 = time.perf_counter()
        want = fr.fullsum_batch_f64(*(v[:n_ref].cpu().numpy() for v in (score, seq, opt, nf, ns)))
        ref_ms = (time.perf_counter() - t0) * 1e3
        e_gamma = float(np.abs(want.state_post - r.state_post[:n_ref].cpu().numpy()).max())
        e_lz = float(np.abs(want.log_z - r.log_z[:n_ref].cpu().numpy()).max())
        assert e_gamma < 64 * F_MAX * 2.0 ** -24, ('the device differs from the reference', e_gamma)
        arms = {'align_posterior_batch (device)': dev_call,
                '(a) align_batch (device)': lambda: ev.align_batch(score, nf, seq, ns, optional=opt, kind='log'),
                '(b) torch, one step per frame': lambda: torch_fullsum(score, seq, opt, nf, ns)}
        times = {k: [] for k in arms}
        for _ in range(a.reps):                                          # interleaved
            for k, f in arms.items():
                times[k].append(timed(f))
        med = {}
        for k, v in times.items():
            med[k] = float(np.median(v))
            say('  %-32s median %10.3f ms  (min %.3f, max %.3f, %d reps)' % (k, med[k], min(v), max(v), len(v)))
        say('  %-32s        %10.3f ms  for %d utterances (wall clock, download included, once): %.0f ms for the batch at that rate'
            % ('(c) tests/fullsum_ref.py, host', ref_ms, n_ref, ref_ms * B / n_ref))
        d = med['align_posterior_batch (device)']
        say('  device against (a): %.2f x the time;  against (b): %.0f x faster;  against (c): %.0f x faster;  %.3f us per frame step of '
            'the batch (both passes), %.2f ns per cell' % (d / med['(a) align_batch (device)'], med['(b) torch, one step per frame'] / d,
                                                           ref_ms * B / n_ref / d, d * 1e3 / F_MAX, d * 1e6 / (float(nf.sum()) * S)))
        say('  max |gamma - gamma64| %.3e, max |log_z - log_z64| %.3e on those %d utterances;  torch form against the device: gamma %.3e, '
            'log_z %.3e' % (e_gamma, e_lz, n_ref, d_gamma, d_lz))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
