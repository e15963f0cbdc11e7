"""MX-FP8 against bf16 inference on one box, in one process, interleaved (ABAB...): the decoder forward at 64 windows
(shipped hyper-parameters, seeded weights) and the step-2 filter-bank launch alone (bank256_kernel vs mx8_conv_kernel,
same shape; the MX launch is timed without the quantisation of its input, which runs as its own small launch), plus
the step-2 projection conv1d_1 alone.  HIP events, warm-ups, >= 20 iterations per sample.  Prints one JSON line.
python tools/ab_mxfp8.py [--windows 64] [--iters 20] [--reps 3]"""
import argparse
import contextlib
import io
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd')):
    sys.path.insert(0, p)
import numpy as np
import torch
import _vc
import modules
import mx8
from oracle import model_oracle as mo

MX_PEAK, BF16_PEAK = 5.0e15, 2.5e15            # dense matrix peaks (FLOP/s)
BANK2_MAC, PROJ2_MAC = 17301504, 3145728        # MAC per frame: step-2 bank (K = 32, Cin 256), step-2 conv1d_1


def timed(fn, n):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    W, T = a.windows, 400
    from decoder import decoder_specs
    cfg = json.load(open(os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'decoder_cfg_d.json')))
    cfg['is_training'] = False
    wd = mo.init_weights(cfg, 'decoder', seed=2, perturb_bn=True)
    decs = {}
    for dt in ('bfloat16', 'mxfp8'):
        with contextlib.redirect_stdout(io.StringIO()):
            decs[dt] = decoder_specs(dict(cfg, compute_dtype=dt), None, None)
        decs[dt].store.load_dict(dict(wd), strict=False)
    rng = np.random.RandomState(0)
    x = torch.softmax(torch.from_numpy(rng.standard_normal((W, T, 61)) * 3.0), -1).float().cuda()
    # stage-2 bank input and the MX operands of both stage-2 launches
    pre = torch.randn(W, T, 256, generator=torch.Generator().manual_seed(1)).cuda().bfloat16()
    runs = {}
    for dt, dec in decs.items():
        st = dec.store
        runs['decoder_' + dt] = lambda dec=dec: dec.forward(x)
        with modules.variable_store(st), modules.variable_scope('decoder/step2/CBHG'):
            if dt == 'bfloat16':
                runs['bank_bf16'] = lambda st=st: _in(st, lambda: modules.conv1d_banks(pre, K=32, is_training=False, pool_output='auto'))
                enc, _ = modules.conv1d_banks(pre, K=32, is_training=False, pool_output='auto')
                runs['proj_bf16'] = lambda st=st, enc=enc: _in(st, lambda: modules.conv1d(
                    enc, filters=256, size=3, scope='conv1d_1', bn_scope='conv1d_1', activation_fn='relu', pool_input=0))
            else:
                mxt, pooled = modules.conv1d_banks(pre, K=32, is_training=False, pool_output='auto', mx8_out=True)
                assert pooled and isinstance(mxt, mx8.MxTensor)
                packed = st._cache[('mx8bank', 'decoder/step2/CBHG/conv1d_banks')]
                s, sh = modules._prep_bn(st, 'decoder/step2/CBHG/conv1d_banks/bn', 4096)
                xq, xs = mx8.quantize(pre.view(W * T, 256), W * T, 256)
                out = torch.empty((W, T, 4096), dtype=torch.uint8, device='cuda')
                outs = torch.empty((W, T, 128), dtype=torch.uint8, device='cuda')
                runs['bank_mx8'] = lambda: mx8._launch(xq, xs, W * T, T, 256, mx8.bank_groups(packed, 32, 256), s, sh,
                                                       _vc.ACT_RELU, 1, _vc.MX8_OUT_MX, 4096, out, outs)
                runs['bank_mx8_quantize'] = lambda: mx8.quantize(pre.view(W * T, 256), W * T, 256)
                runs['proj_mx8'] = lambda st=st, mxt=mxt: _in(st, lambda: modules.conv1d(
                    mxt, filters=256, size=3, scope='conv1d_1', bn_scope='conv1d_1', activation_fn='relu'))
    samples = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            samples[k].append(timed(fn, a.iters))
    ms = {k: float(np.median(v)) for k, v in samples.items()}
    M = W * T
    res = {'windows': W, 'iters': a.iters, 'reps': a.reps, 'ms': ms,
           'ms_spread': {k: [float(min(v)), float(max(v))] for k, v in samples.items()},
           'decoder_frames_per_s': {dt: M / (ms['decoder_' + dt] / 1e3) for dt in decs},
           'decoder_speedup': ms['decoder_bfloat16'] / ms['decoder_mxfp8'],
           'bank_speedup': ms['bank_bf16'] / ms['bank_mx8'],
           'bank_mx8_tflops': 2.0 * BANK2_MAC * M / (ms['bank_mx8'] / 1e3) / 1e12,
           'bank_mx8_share_of_mx_peak': 2.0 * BANK2_MAC * M / (ms['bank_mx8'] / 1e3) / MX_PEAK,
           'bank_bf16_share_of_bf16_peak': 2.0 * BANK2_MAC * M / (ms['bank_bf16'] / 1e3) / BF16_PEAK,
           'proj_mx8_tflops': 2.0 * PROJ2_MAC * M / (ms['proj_mx8'] / 1e3) / 1e12,
           'proj_mx8_share_of_mx_peak': 2.0 * PROJ2_MAC * M / (ms['proj_mx8'] / 1e3) / MX_PEAK,
           'proj_speedup': ms['proj_bf16'] / ms['proj_mx8']}
    print(json.dumps(res))


def _in(st, fn):
    with modules.variable_store(st), modules.variable_scope('decoder/step2/CBHG'):
        return fn()


if __name__ == '__main__':
    main()
