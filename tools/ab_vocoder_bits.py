"""Bit-equality record of the STFT-domain launches of csrc/vc_vocoder.hip: a fixed list of calls on fixed seeded inputs, one
SHA-256 per returned tensor (the Griffin-Lim trace, a sum of float atomics, as four significant digits).  Run it on a build
of the parent commit and on this tree; the two files must be identical.

Entry points: vc_griffin_lim_f32 (3 iterations), vc_griffin_lim_momentum_f32 (momentum 0.99, 4 iterations, trace on),
vc_stft_filter_f32, vc_stft_power_f32, vc_stft_complex_f32, vc_istft_complex_f32 (on the spectrum the line before returned).
Shapes: n_fft 400, hop 80 at 1, 15, 16, 17 and 33 frames (partial tile, full tile, tile seam) and a batch of three (33 and 7
frames and one utterance shorter than n_fft / 2: the "short" rule and the zero-row writers); the generic path at n_fft 16,
hop 4 with 3, 4, 5 and 9 frames and at n_fft 512, hop 128 with 9.  A call the entry point refuses (Griffin-Lim on frames
shorter than the reflect padding) is recorded by its error text.

    python tools/ab_vocoder_bits.py --out profiles/vocoder_halves/bits_this.txt
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd')):
    sys.path.insert(0, p)

# (n_fft, hop, frames per utterance, the short utterance's samples or None)
CASES = [(400, 80, [f], None) for f in (1, 15, 16, 17, 33)] + [(400, 80, [33, 7, 4], 150)] + \
        [(16, 4, [f], None) for f in (3, 4, 5, 9)] + [(512, 128, [9], None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import _vc
    import audio_lib
    if not torch.cuda.is_available():
        raise SystemExit('ab_vocoder_bits needs a GPU')
    lines = []

    def record(case, entry, **tensors):
        for name, t in tensors.items():
            if name == 'trace':                        # summed with float atomics: the order, and so the last bits, vary run to run
                lines.append('%-22s %-28s %-8s %s' % (case, entry, name, ' '.join('%.3e' % v for v in t.flatten().tolist())))
                continue
            h = hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()
            lines.append('%-22s %-28s %-8s %-16s %s' % (case, entry, name, 'x'.join(map(str, t.shape)), h))

    def attempt(case, entry, fn):
        try:
            out = fn()
        except (_vc.VCError, ValueError) as e:
            lines.append('%-22s %-28s refused: %s' % (case, entry, str(e).splitlines()[0]))
            return None
        record(case, entry, **out)
        return out

    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')
    for ci, (n_fft, hop, frames, short) in enumerate(CASES):
        case = 'n%d_h%d_f%s' % (n_fft, hop, '-'.join(map(str, frames)))
        g = torch.Generator().manual_seed(1000 + ci)
        B, Fmax, nb = len(frames), max(frames), 1 + n_fft // 2
        plan = audio_lib._get_voc_plan(n_fft, hop, n_fft)
        rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
        # Griffin-Lim: magnitudes and a start phase; frame counts only for the batch
        amp, ph = (rnd(B, Fmax, nb) + 0.05).cuda(), (np.pi * rnd(B, Fmax, nb)).cuda()
        d_nf = i32(frames) if B > 1 else None
        attempt(case, 'vc_griffin_lim_f32', lambda: {'wav': audio_lib._griffin_lim_launch(plan, amp, ph, d_nf, 3, False, 0.0)})
        attempt(case, 'vc_griffin_lim_momentum_f32',
                lambda: dict(zip(('wav', 'trace'), audio_lib._griffin_lim_launch(plan, amp, ph, d_nf, 4, True, 0.99))))
        # the waveform launches: utterance b holds hop * (frames - 1) samples, the short one `short`
        lens = [hop * (f - 1) for f in frames]
        if short is not None:
            lens[-1] = short
        Lmax = max(max(lens), 1)
        wav = (rnd(B, Lmax) - 0.5).cuda()
        d_len = i32(lens)
        gain = (rnd(B, max(Fmax, 2), nb) * 2.0).cuda()
        if Fmax >= 2:
            attempt(case, 'vc_stft_filter_f32', lambda: {'y': audio_lib._stft_filter_launch(plan, wav, d_len, gain, None)})
        attempt(case, 'vc_stft_power_f32',
                lambda: dict(zip(('power', 'frames'), audio_lib._stft_power_launch(plan, wav, d_len, None, Fmax))))
        z = attempt(case, 'vc_stft_complex_f32',
                    lambda: dict(zip(('re', 'im', 'frames'), audio_lib._stft_complex_launch(plan, wav, d_len, None, Fmax))))
        if z is not None:
            attempt(case, 'vc_istft_complex_f32',
                    lambda: {'y': audio_lib._istft_complex_launch(plan, z['re'], z['im'], z['frames'])})
    torch.cuda.synchronize()
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
