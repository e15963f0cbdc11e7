"""Measurements of the content scores (csrc/vc_content.hip) on one MI355X.

Models: the small float32 test models (the golden encoder checkpoint, a decoder with seeded RANDOM weights), so the
figures show that the plumbing works, not the quality of a conversion.  Input: 16 utterances of 5 s of synthetic speech.

  default        wall time of content_batch on the posteriors of one content_wav_batch (HIP events, interleaved with the
                 same figures computed by tests/content_ref.py on the host from downloaded tensors), then frame_agreement,
                 js_mean and per of a bf16 and of an mxfp8 conversion against the float32 one
  --kernel-only  a few content_wav_batch calls and nothing else: for a kernel trace

    python tools/ab_content.py --reps 9 --out profiles/content/ab_content.log
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/ab_content.py --kernel-only --reps 3
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def models(kind='float32'):
    """(decoder, encoder to pass to convert_batch or None, encoder that made the posteriors, data-set configuration)."""
    from decoder import decoder_specs
    from encoder import encoder_spec_phn
    from oracle import model_oracle as mo
    from test_conversion_gpu import _cfgs
    enc_cfg, dec_cfg, c = _cfgs(os.path.join(ROOT, 'tests', 'golden'))
    wd = mo.init_weights(dec_cfg, 'decoder', seed=2, perturb_bn=True)
    if kind != 'float32':
        enc_cfg, dec_cfg = dict(enc_cfg, compute_dtype='bfloat16'), dict(dec_cfg, compute_dtype=kind)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
        dec = decoder_specs(dec_cfg, None, None if kind == 'mxfp8' else enc)
        if kind == 'mxfp8':
            enc.restore()
    dec.store.load_dict(dict(wd), strict=False)
    return dec, (enc if kind == 'mxfp8' else None), enc, c


def host_content(ppg_a, ppg_b, la, lb, cmap, min_run=3):
    """content_batch's figures by tests/content_ref.py, pair by pair."""
    import content_ref as cr
    out = []
    for b in range(len(la)):
        m = cr.ppg_metrics(ppg_a[b], ppg_b[b], la[b], lb[b], None, cmap)
        sa, sb = cr.phn_segments(ppg_a[b], la[b], cmap, min_run)[0], cr.phn_segments(ppg_b[b], lb[b], cmap, min_run)[0]
        out.append((m, cr.edit_distance(sa, sb)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    import torch
    import conversion
    import evaluation as ev
    import sound_ds
    from oracle import frontend_oracle as fo
    if not torch.cuda.is_available():
        raise SystemExit('ab_content needs a GPU')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, L = 16, 5 * 16000
    wav = np.stack([fo.synth_speech(1, L, seed=70 + b)[0] for b in range(B)]).astype(np.float32)
    lens = [L] * B
    cmap = ev.class_map(sound_ds.TIMIT_PHONEMES_61)
    dec, _, enc, c = models('float32')
    ref = conversion.convert_batch(dec, wav, lens, c, n_iter=32, momentum=0.99, seed=1)
    y, ny = ref.y_wav_pred, ref.n_samples
    d_wav = torch.from_numpy(wav).cuda()
    call = lambda: ev.content_wav_batch(enc, d_wav, lens, y, ny, c, class_map=cmap, ppg_a=None)
    r = call()
    torch.cuda.synchronize()
    if a.kernel_only:
        for _ in range(a.reps):
            call()
        torch.cuda.synchronize()
        return
    la, lb = r.len_a.cpu().tolist(), r.len_b.cpu().tolist()
    say('%d utterances of 5 s, source against its own float32 conversion (32 fast Griffin-Lim iterations), RANDOM decoder weights:' % B)
    say('  posteriors [%d, %d, %d] and [%d, %d, %d]; frames scored %s' % (*r.ppg_a.shape, *r.ppg_b.shape, sorted(set(zip(la, lb)))))
    say('  frame_agreement %.4f  js_mean %.4f bit  per %.4f  (means over the batch; %d and %d segments in the first pair)'
        % (float(r.frame_agreement.mean()), float(r.js_mean.mean()), float(r.per.mean()), int(r.seg_a.n_seg[0]), int(r.seg_b.n_seg[0])))
    dev = lambda: ev.content_batch(r.ppg_a, r.ppg_b, la, lb, class_map=cmap)
    dev()
    torch.cuda.synchronize()
    t_dev, t_host = [], []
    for k in range(a.reps):                                              # interleaved; the host arm fewer times: it takes seconds
        t0 = time.perf_counter()
        dev()
        torch.cuda.synchronize()
        t_dev.append(1e3 * (time.perf_counter() - t0))
        if k < 3:
            t0 = time.perf_counter()
            h = host_content(r.ppg_a.cpu().numpy(), r.ppg_b.cpu().numpy(), la, lb, cmap)
            t_host.append(1e3 * (time.perf_counter() - t0))
    say('  content_batch on those posteriors, host clock to a device synchronise: median %.3f ms (min %.3f, max %.3f, %d reps)'
        % (float(np.median(t_dev)), min(t_dev), max(t_dev), len(t_dev)))
    say('  the same figures by tests/content_ref.py on the host from downloaded tensors: median %.1f ms (min %.1f, %d reps)'
        % (float(np.median(t_host)), min(t_host), len(t_host)))
    worst = max(abs(float(r.js_mean[b]) - h[b][0]['js_mean']) for b in range(B))
    same = all(int(r.dist[b]) == h[b][1]['dist'] and int(r.n_agree[b]) == h[b][0]['n_agree'] for b in range(B))
    say('  device against host: counts and distances equal: %s; largest js_mean difference %.2e' % (same, worst))
    for kind in ('bfloat16', 'mxfp8'):
        dk, enc_arg, enc_k, _ = models(kind)
        rk = conversion.convert_batch(dk, wav, lens, c, n_iter=32, momentum=0.99, seed=1, encoder=enc_arg)
        s = ev.content_wav_batch(enc, y, ny, rk.y_wav_pred, rk.n_samples, c, class_map=cmap)
        say('  %-8s conversion against the float32 one (float32 encoder on both waveforms, RANDOM decoder weights): frame_agreement '
            '%.4f  js_mean %.4f bit  per %.4f' % (kind, float(s.frame_agreement.mean()), float(s.js_mean.mean()), float(s.per.mean())))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
