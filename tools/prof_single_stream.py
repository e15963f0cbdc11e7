#!/usr/bin/env python
"""The latency-bound caller for rocprofv3: front-end + encode + decode of 64 windows, one batch at a time on one stream,
with the library's defaults (what bench.py --full reports as single_stream).

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_single_stream.py [forwards]

The first forward builds every weight-layout copy (the recurrent-weight images among them: one pack launch per GRU
scope and form); the remaining forwards are the steady state.  Prints the HIP-event time of a steady-state forward."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'speech-cloner_amd')):
    sys.path.insert(0, p)
import torch          # noqa: E402
import audio_lib      # noqa: E402
import bench          # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
wav = bench.synth_audio(32, 64000, 0).cuda()
enc, dec = bench.load_models('bfloat16', 0)
fe = None
ms = []
for i in range(n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fe = audio_lib.calc_MFCC_input_batch(wav, None, out=fe, out_frames=800, **bench.FE_KW)
    dec.forward(fe[0].view(64, 400, 80))
    b.record()
    torch.cuda.synchronize()
    ms.append(a.elapsed_time(b))
print('single-stream step (front-end + encode + decode of 64 windows), %d forwards: first %.3f ms, median of the rest %.3f ms'
      % (n, ms[0], sorted(ms[1:])[(n - 1) // 2]))
