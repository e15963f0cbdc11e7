"""Measurements of the exemplar launches (csrc/vc_knn.hip) on one MI355X.

Input: seeded peaky posteriors (tests/exemplar_ref.py) and random values -- the figures are times, not scores.

  default        HIP-event times of vc_knn_i8 (sweep + merge) and of vc_knn_mean_f32 at Mq = 16 x 1,001 queries, C = 61, N = 30 k /
                 120 k / 480 k bank rows, k = 4 and 16, interleaved with the baseline on the same data in the same process:
                 chunked torch float32 matmul + topk + merge over the float images of the same int8 keys (exact below 2^24, so
                 it returns the same distances; its tie order is torch's).  Then the key launch, a small-batch point
                 (Mq = 100), and wall times of convert_knn_diff_batch against convert_diff_batch and convert_gmm_diff_batch at
                 16 x 5 s.
  --kernel-only  a few searches and means and nothing else: for a kernel trace or a counter run

    python tools/ab_knn.py --reps 9 --out profiles/knn/ab_knn.log
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

INT8_MAC_PER_S = 2.5e15         # MI355X dense int8: ~5 POP/s = 2.5e15 multiply-adds per second
HBM_BYTES_PER_S = 8.0e12


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
    return out


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
    return out


def fmt(ts):
    return '%.4f / %.4f / %.4f' % (float(np.median(ts)), min(ts), max(ts))


def torch_knn(qf, qn, bf, bn, k, chunk):
    """Chunked float32 matmul + topk + merge: distances of the same integer keys, exact in float32 (every value < 2^24)."""
    import torch
    best_d = best_j = None
    for s in range(0, bf.shape[0], chunk):
        e = min(bf.shape[0], s + chunk)
        d = qn[:, None] + bn[None, s:e] - 2.0 * (qf @ bf[s:e].T)
        dk, jk = torch.topk(d, min(k, e - s), dim=1, largest=False)
        jk = jk + s
        if best_d is None:
            best_d, best_j = dk, jk
        else:
            cd, cj = torch.cat([best_d, dk], 1), torch.cat([best_j, jk], 1)
            best_d, at = torch.topk(cd, k, dim=1, largest=False)
            best_j = torch.gather(cj, 1, at)
    return best_d, best_j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--banks', default='30000,120000,480000')
    ap.add_argument('--no-convert', action='store_true')
    a = ap.parse_args()
    import torch
    import _vc
    import exemplar
    import exemplar_ref as er
    if not torch.cuda.is_available():
        raise SystemExit('ab_knn needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, F, C = 16, 1001, 61
    Mq = B * F
    nf = [F] * B
    d_nf = torch.tensor(nf, dtype=torch.int32, device='cuda')
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    q_ppg = cuda(er.peaky_posteriors(Mq, C, seed=1).reshape(B, F, C))
    keys, norms = exemplar._key_launch(q_ppg, d_nf)
    banks = [int(v) for v in a.banks.split(',')]
    rng = np.random.RandomState(0)

    def make_bank(N):
        p = cuda(er.peaky_posteriors(N, C, seed=2)[None])
        bk, bn = exemplar._key_launch(p, torch.tensor([N], dtype=torch.int32, device='cuda'))
        V = cuda(rng.standard_normal((N, 201)).astype(np.float32))
        return exemplar.Bank(bk[0].contiguous(), bn[0].contiguous(), V, V[:, :80].contiguous(), None, None, None, C)

    if a.kernel_only:
        bank = make_bank(banks[min(1, len(banks) - 1)])
        for k in (4, 16):
            for _ in range(a.reps):
                idx, dist = exemplar._knn_launch(keys, norms, d_nf, None, None, bank, k, 0)
                exemplar._mean_launch(idx, dist, bank.stft, -1)
        torch.cuda.synchronize()
        return

    say('vc_ppg_key_i8, %d x %d x %d (median / min / max of %d, HIP events, ms): %s' % (B, F, C, a.reps, fmt(event_ms(lambda: exemplar._key_launch(q_ppg, d_nf), a.reps))))
    qf, qnf = keys.reshape(Mq, -1).float(), norms.reshape(Mq).float()
    for N in banks:
        bank = make_bank(N)
        bf, bnf = bank.key.float(), bank.norm.float()
        chunk = min(N, 32768)                               # the [Mq, chunk] float32 score block: 2.1 GB
        for k in (4, 16):
            ns = int(_vc.lib().vc_knn_splits(Mq, N, 0))
            ws = torch.empty((exemplar.workspace_bytes(Mq, N, k),), dtype=torch.uint8, device='cuda')
            ours = lambda: exemplar._knn_launch(keys, norms, d_nf, None, None, bank, k, 0, ws)
            base = lambda: torch_knn(qf, qnf, bf, bnf, k, chunk)
            idx, dist = ours()
            bd, _ = base()
            agree = bool(torch.equal(dist.reshape(Mq, k).float(), bd))
            t_o, t_b = [], []
            for _ in range(a.reps):                         # interleaved: one of each per round
                t_o += event_ms(ours, 1)
                t_b += event_ms(base, 1)
            mean = lambda: exemplar._mean_launch(idx, dist, bank.stft, -1)
            t_m = event_ms(mean, a.reps)
            macs = float(Mq) * N * 64
            med = float(np.median(t_o)) * 1e-3
            say('Mq = %d, N = %d, k = %d, %d splits (median / min / max of %d, ms): vc_knn_i8 %s; torch float32 matmul + topk + merge '
                '(chunks of %d) %s; ratio %.2f; distances agree: %s' % (Mq, N, k, ns, a.reps, fmt(t_o), chunk, fmt(t_b),
                                                                       float(np.median(t_b)) / float(np.median(t_o)), agree))
            say('    %.3g int8 MACs: %.1f us at the dense int8 line, %.1f %% of it achieved; %.3g candidates: %.2f ns per 1,000 candidates; '
                'bank bytes once %.1f MB' % (macs, 1e6 * macs / INT8_MAC_PER_S, 100 * macs / INT8_MAC_PER_S / med, float(Mq) * N,
                                             1e9 * med / (float(Mq) * N / 1e3), N * 68 / 1e6))
            gb = Mq * (k + 1) * 201 * 4
            say('    vc_knn_mean_f32, D = 201: %s ms; moves %.1f MB: %.1f %% of the HBM line' % (fmt(t_m), gb / 1e6,
                                                                                                 100 * gb / HBM_BYTES_PER_S / (float(np.median(t_m)) * 1e-3)))
        del bank, bf, bnf
    # a small batch: the grid is filled by splits
    bank = make_bank(banks[min(1, len(banks) - 1)])
    N = bank.key.shape[0]
    k1, n1 = keys[:1, :100].contiguous(), norms[:1, :100].contiguous()
    d1 = torch.tensor([100], dtype=torch.int32, device='cuda')
    say('Mq = 100, N = %d, k = 4, %d splits: vc_knn_i8 %s ms' % (N, int(_vc.lib().vc_knn_splits(100, N, 0)),
                                                                fmt(event_ms(lambda: exemplar._knn_launch(k1, n1, d1, None, None, bank, 4, 0), a.reps))))
    if not a.no_convert:
        import ab_convert_batch as acb
        import conversion
        import mapping
        import mapping_ref as mr
        from bench import synth_audio
        dec, c = acb.models()
        L = 5 * c['sample_rate']
        wav = synth_audio(16, L, seed=300).float().cuda()
        m = mr.random_model(32, 48, seed=2, spread=0.5)
        model = mapping.JDGMM(*(cuda(m[key]) for key in mr.FIELDS))
        tk = wall_ms(lambda: conversion.convert_knn_diff_batch(bank, wav, None, c, encoder=dec.encoder, k=4), a.reps)
        td = wall_ms(lambda: conversion.convert_diff_batch(dec, wav, None, c), a.reps)
        tg = wall_ms(lambda: conversion.convert_gmm_diff_batch(model, wav, None, c), a.reps)
        say('16 x 5 s, host clock to a device synchronise (median / min / max, ms): convert_knn_diff_batch (encoder, bank of %d, k = 4) %s; '
            'convert_diff_batch (encoder + decoder) %s; convert_gmm_diff_batch (M = 32, 24 cepstra) %s' % (N, fmt(tk), fmt(td), fmt(tg)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
