"""How precisely v_mfma_scale_f32_32x32x64_f8f6f4 sums its products -- the basis of the kernel tolerance of
tests/test_mx8_gpu.py (log: profiles/mx8/mfma_accumulation_diag.log).

Raw filter-bank convolutions (no BN, relu or pool: epilogue scale 1, shift 0, float32 output) of seeded data through
vc_mx8_conv, against float64 of the device's own quantised operands; once as they are and once with every e4m3
subnormal of both operands flushed to zero in the reference.  Printed per case: max |err|, mean err, and the largest
err / sum |a w| (the width-1 filter of K = 2 takes two MFMAs and an exact epilogue, so its error is the instruction's).
python tools/mx8_mfma_accumulation.py"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np
import torch
import _vc
import mx8
import mx8_ref as mx
from oracle import model_oracle as mo


def _np(t):
    return t.detach().cpu().numpy()


def main():
    for K, Cin in ((2, 128), (32, 256)):
        rng = np.random.RandomState(0)
        N, T = 3, 400
        x = torch.from_numpy(rng.standard_normal((N, T, Cin)).astype(np.float32)).cuda().bfloat16()
        kern = [torch.from_numpy(rng.uniform(-0.06, 0.06, (k, Cin, 128)).astype(np.float32)).cuda() for k in range(1, K + 1)]
        packed = [mx8.pack_kernel(k) for k in kern]
        one, zero = torch.ones(128 * K, device='cuda'), torch.zeros(128 * K, device='cuda')
        xq, xs = mx8.quantize(x.view(N * T, Cin), N * T, Cin)
        out = torch.empty((N, T, 128 * K), device='cuda')
        mx8._launch(xq, xs, N * T, T, Cin, mx8.bank_groups(packed, K, Cin), one, zero, _vc.ACT_NONE, 0, _vc.MX8_OUT_F32,
                    128 * K, out)
        xc, xsc = _np(xq), _np(xs)
        for flush in (False, True):
            xd = mx.dequantize(np.where(flush & ((xc & 0x78) == 0), 0, xc), xsc).reshape(N, T, Cin)
            ref, absr = [], []
            for k, (w, ws) in zip(range(1, K + 1), packed):
                wc = _np(w)
                wc = np.where(flush & ((wc & 0x78) == 0), 0, wc)
                wd = torch.from_numpy(mx.dequantize(wc, _np(ws)).T.reshape(k, Cin, 128).copy())
                ref.append(mo.conv1d(torch.from_numpy(xd), wd))
                absr.append(mo.conv1d(torch.from_numpy(np.abs(xd)), wd.abs()))
            ref, absr = torch.cat(ref, -1).numpy(), torch.cat(absr, -1).numpy()
            err = _np(out).astype(np.float64) - ref
            rel = np.abs(err) / np.maximum(absr, 1e-30)
            print('K=%d Cin=%d flush=%d: max|err| %.3e  mean err %.3e  max err/sum|aw| %.3e (= 2^%.1f)  p99.9 %.3e'
                  % (K, Cin, flush, np.abs(err).max(), err.mean(), rel.max(), np.log2(rel.max()), np.quantile(rel, 0.999)))


if __name__ == '__main__':
    main()
