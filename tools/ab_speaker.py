"""Measurements of the speaker-similarity launches (csrc/vc_gmm.hip) on one MI355X.

Input: random features, 64 utterances of 1,000 frames, D = 48 -- the figures are times, not scores.

  default        per launch of one EM iteration (prepare, loglik, accumulate + reduce, update) at M = 64 and 256: HIP-event
                 times, and for the accumulate launch the bytes and FLOPs it must move and do with the share of the HBM and
                 float32 lines its time stands for; then gmm_score_batch at 16 x 1,000 frames against tests/speaker_ref.py
                 on the host
  --kernel-only  a few gmm_fit calls and nothing else: for a kernel trace

    python tools/ab_speaker.py --reps 9 --out profiles/speaker/ab_speaker.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_speaker.py --kernel-only --reps 3
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12        # MI355X: 8 TB/s
F32_FLOPS = 157.3e12            # vector float32 peak


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    import speaker as sp
    import speaker_ref as sr
    if not torch.cuda.is_available():
        raise SystemExit('ab_speaker needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    B, F, D = 64, 1000, 48
    x = torch.from_numpy(rng.standard_normal((B, F, D)).astype(np.float32)).cuda()
    lens = [F] * B
    if a.kernel_only:
        for _ in range(a.reps):
            sp.gmm_fit(x, lens, 64, 4)
        torch.cuda.synchronize()
        return
    d_len = torch.tensor(lens, dtype=torch.int32, device='cuda')
    zeros = torch.zeros(B, dtype=torch.int32, device='cuda')
    for M in (64, 256):
        ubm, _ = sp.gmm_fit(x, lens, M, 2)
        w, mu, var = ubm
        floor = torch.full((D,), 1e-3, device='cuda')
        tab = sp._prepare_launch(w, mu[None], var)
        ll = sp._loglik_launch(x, d_len, tab, 1, M, zeros)[0]
        ws = torch.empty(max(sp.workspace_bytes(1, M, D), 1), dtype=torch.uint8, device='cuda')
        st = sp._accumulate_launch(x, ll, d_len, None, zeros, tab, 1, M, 1, ws=ws)
        say('one EM iteration, %d x %d frames, D = %d, M = %d (median / min / max of %d, HIP events, ms):' % (B, F, D, M, a.reps))
        t = {}
        t['prepare'] = event_ms(lambda: sp._prepare_launch(w, mu[None], var), a.reps)
        t['loglik'] = event_ms(lambda: sp._loglik_launch(x, d_len, tab, 1, M, zeros), a.reps)
        t['accumulate'] = event_ms(lambda: sp._accumulate_launch(x, ll, d_len, None, zeros, tab, 1, M, 1, ws=ws), a.reps)
        t['update'] = event_ms(lambda: sp._update_em_launch(st, mu, var, floor, 1.0), a.reps)
        for k, v in t.items():
            say('  %-10s %.4f / %.4f / %.4f' % (k, *v))
        chunks = (M + 63) // 64
        n = B * F
        must_bytes = chunks * n * (D + 1) * 4 + 2 * sp.workspace_bytes(1, M, D)         # features and ll once per chunk; partials written, read
        flops = n * M * (3 * D + 2) + n * M * (4 * D + 1) * 2                        # gamma (float32) + the float64 folds counted as 2
        sec = t['accumulate'][0] * 1e-3
        say('  accumulate must move %.1f MB and do %.2f GFLOP: %.1f %% of the HBM line, %.1f %% of the float32 line'
            % (must_bytes / 1e6, flops / 1e9, 100 * must_bytes / HBM_BYTES_PER_S / sec, 100 * flops / F32_FLOPS / sec))
    # scoring against the host
    Bs = 16
    ubm, _ = sp.gmm_fit(x, lens, 64, 2)
    means = sp.gmm_adapt_batch(ubm, x, lens, [b % 4 for b in range(B)], 4)
    idx = [b % 4 for b in range(Bs)]
    dev = lambda: sp.gmm_score_batch(ubm, means, x[:Bs], lens[:Bs], idx)
    r = dev()
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        dev()
        torch.cuda.synchronize()
        t_dev.append(1e3 * (time.perf_counter() - t0))
    hw, hm, hv, hs, hx = (t.cpu().numpy() for t in (*ubm, means, x[:Bs]))
    t0 = time.perf_counter()
    host = [sr.score(sr.loglik(hx[b], hw, hs[idx[b]], hv)[0], sr.loglik(hx[b], hw, hm, hv)[0], F)[3] for b in range(Bs)]
    t_host = 1e3 * (time.perf_counter() - t0)
    say('gmm_score_batch, %d x %d frames, M = 64, host clock to a device synchronise: median %.3f ms (min %.3f, max %.3f, %d reps)'
        % (Bs, F, float(np.median(t_dev)), min(t_dev), max(t_dev), len(t_dev)))
    say('the same LLRs by tests/speaker_ref.py on the host (float64, one run): %.1f ms; largest difference %.2e'
        % (t_host, float(np.abs(r.llr.cpu().numpy() - np.array(host)).max())))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
