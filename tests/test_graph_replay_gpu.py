"""Graph capture and replay of the library's launches (include/vc_hip.h: every launch call is hipGraph-capturable).

A captured graph freezes every launch argument and every host-side decision of the capture.  A launch that keeps state
between launches (arrival counters, tickets, READY words) must therefore re-initialise it inside the graph, and a
replay must compute what an eager call computes on the same inputs.  Each test here:
  * warms the call up eagerly before the capture, so that plans and weight-layout caches exist;
  * captures ONE stream (no forked streams; decoder.predict(n_streams > 1) is never captured), with no host <-> device
    copy inside the capture: lengths and initial phases are device tensors, outputs are preallocated or graph-owned;
  * replays with NEW inputs copied into the static input tensors before each replay (a replay that reused the state or
    the statistics of the previous replay would pass a check against the same input);
  * asserts each replay bit-identical to an eager call on the same inputs (inference is run-to-run deterministic,
    test_model_gpu.py), and where a test already fixes an independent reference, within its bound of that too;
  * frees its graphs at the end.
The vocoder's trace is the one exception to bit identity: it sums squares with float atomicAdd in no fixed order, so it
is compared with a relative bound of 1e-5."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import fgla_ref as fr
from conftest import FE_KW, GOLDEN, ROOT
from oracle import frontend_oracle as fo
from oracle import vocoder_oracle as vo

pytestmark = pytest.mark.gpu

TOL = {'mfcc': 1e-4, 'mel': 1e-4, 'pdb': 2e-4}      # test_frontend_gpu.py: the front-end's bounds against the oracle
# One launch against two (test_frontend_gpu.py): identical extremes, sum|x| in another order, so the dB values differ by
# roundings: 2e-6 for mel and power dB.  The MFCC half sums 80 of them per cepstrum and its delta half is 2 (c[t+1] -
# c[t-1]): twice that bound (measured up to 2.4e-6 on the audio of these tests).
FORM_TOL = {'mfcc': 4e-6, 'mel': 2e-6, 'pdb': 2e-6}
FE_NAMES = ('mfcc', 'mel', 'pdb')
HP = os.path.join(ROOT, 'speech-cloner_amd', 'hp')


def _capture(fn):
    """One eager warm-up call of fn on a side stream, then one call captured into a graph; returns (graph, outputs)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    torch.cuda.synchronize()
    return g, out


def _free(*graphs):
    torch.cuda.synchronize()
    for g in graphs:
        g.reset()


def _same(got, want, what):
    """Bit-identical, with the size of the difference in the message when not."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError('%s: not bit-identical to eager: %d of %d values differ, max |diff| %.3e'
                             % (what, int((got != want).sum()), got.numel(), float(d.nan_to_num(float('inf')).max())))


# --------------------------------------------------------------------------------------------- front-end
def _fe_inputs(B, L, k, seed):
    """Replay k's batch: new speech-like audio, a gain per utterance that changes by x4 or x16 from one k to the next
    (so the extremes and mean|x| differ), and ragged lengths that move between the utterances from one k to the next.
    The shortest utterance has 1119 samples (14 frames: one feature tile)."""
    base = [L, L - 1, 1119, L // 2, 3 * L // 4 + 41, L - 80]
    lens = np.array([base[(b + k) % len(base)] if b < len(base) else L - 7 * b for b in range(B)], np.int32)
    wav = fo.synth_speech(B, L, seed=seed + 31 * k)
    gains = 0.01 * 4.0 ** ((np.arange(B) + k) % 3)
    for b in range(B):
        wav[b] *= gains[b]
        wav[b, lens[b]:] = 0.0
    return wav, lens


def _fe_eager(d_wav, d_lens, R):
    import audio_lib
    return tuple(t.clone() for t in audio_lib.calc_MFCC_input_batch(d_wav, d_lens, out_frames=R, **FE_KW))


def _fe_refs(B, L, R, n, seed):
    """Device inputs and eager results (one launch, and the two-launch form) of n front-end batches, all computed
    before any capture (the options are not changed once a graph exists)."""
    import _vc
    cases = []
    for k in range(n):
        wav, lens = _fe_inputs(B, L, k, seed)
        d_wav, d_lens = torch.from_numpy(wav).cuda(), torch.from_numpy(lens).cuda()
        with _vc.options(fe_fused=1):
            one = _fe_eager(d_wav, d_lens, R)
        with _vc.options(fe_fused=0):
            two = _fe_eager(d_wav, d_lens, R)
        cases.append(dict(wav=wav, lens=lens, d_wav=d_wav, d_lens=d_lens, one=one, two=two))
    return cases


def _fe_check(got, case, R, what, oracle=True):
    """got == eager one-launch bit for bit; within FORM_TOL of the two-launch form; within TOL of the float64 oracle for
    the shortest, the longest and one middle utterance."""
    for name, g_, o_, t_ in zip(FE_NAMES, got, case['one'], case['two']):
        _same(g_, o_, '%s %s' % (what, name))
        assert torch.isfinite(g_).all(), (what, name)
        assert float((g_ - t_).abs().max()) < FORM_TOL[name], (what, name, float((g_ - t_).abs().max()))
    if not oracle:
        return
    lens = case['lens']
    for b in sorted({int(np.argmin(lens)), int(np.argmax(lens)), len(lens) // 2}):
        n = int(lens[b])
        rows = min(1 + n // 80, got[0].shape[1])
        ref = fo.calc_MFCC_input(case['wav'][b, :n], **FE_KW)
        for name, g_, r in zip(FE_NAMES, got, ref):
            err = float(np.abs(g_[b, :rows].cpu().numpy().astype(np.float64) - r[:rows]).max())
            assert err <= TOL[name], '%s %s[%d] len %d: max abs err %.3e vs oracle > %.1e' % (what, name, b, n, err,
                                                                                              TOL[name])


class _FeGraph:
    """calc_MFCC_input_batch captured on static [B, L] audio, a static device lens tensor and preallocated outputs."""

    def __init__(self, B, L, R, first):
        import audio_lib
        self.wav = first['d_wav'].clone()
        self.lens = first['d_lens'].clone()
        Rn = R or 1 + L // 80
        self.out = (torch.empty(B, Rn, 80, device='cuda'), torch.empty(B, Rn, 80, device='cuda'),
                    torch.empty(B, Rn, 201, device='cuda'))
        self.graph, _ = _capture(lambda: audio_lib.calc_MFCC_input_batch(self.wav, self.lens, out=self.out,
                                                                        out_frames=R, **FE_KW))

    def replay(self, case):
        self.wav.copy_(case['d_wav'])
        self.lens.copy_(case['d_lens'])
        self.graph.replay()
        torch.cuda.synchronize()
        return self.out


@pytest.mark.parametrize('B,L,R', [(6, 16000, None), (6, 64000, 800), (32, 64000, 800)],
                         ids=['6x1s_all_rows', '6x4s_800_rows', 'bench_32x4s_800_rows'])
def test_frontend_one_launch_graph_replays_with_new_audio(B, L, R):
    """The default one-launch front-end (fe400_fused_kernel) keeps per-utterance arrival counters and READY words.
    Replayed four times with new audio, gains and lengths, every replay must compute the eager result.  Counters that
    are not re-initialised by the graph itself let replay 2's waiters through at once, onto replay 1's statistics."""
    import _vc
    with _vc.options(fe_fused=1):
        cases = _fe_refs(B, L, R, 4, seed=100 + B)
        fg = _FeGraph(B, L, R, cases[0])
        try:
            for k, case in enumerate(cases):
                _fe_check(fg.replay(case), case, R, 'replay %d' % (k + 1))
        finally:
            _free(fg.graph)


def test_frontend_graph_with_eager_calls_between_replays():
    """Eager calls of the same plan interleaved with the replays (each eager call used to flip the plan's counter
    parity behind the graph's back), then two replays back to back."""
    import _vc
    B, L = 6, 16000
    with _vc.options(fe_fused=1):
        cases = _fe_refs(B, L, None, 4, seed=7)
        fg = _FeGraph(B, L, None, cases[0])
        try:
            _fe_check(fg.replay(cases[0]), cases[0], None, 'replay 1')
            _fe_check(_fe_eager(cases[1]['d_wav'], cases[1]['d_lens'], None), cases[1], None, 'eager', oracle=False)
            _fe_check(fg.replay(cases[2]), cases[2], None, 'replay 2 after an eager call')
            _fe_check(fg.replay(cases[3]), cases[3], None, 'replay 3')
            _fe_check(_fe_eager(cases[0]['d_wav'], cases[0]['d_lens'], None), cases[0], None, 'eager again',
                      oracle=False)
            _fe_check(fg.replay(cases[1]), cases[1], None, 'replay 4 after an eager call')
        finally:
            _free(fg.graph)


def test_frontend_two_graphs_of_one_plan_replayed_alternately():
    import _vc
    B, L = 6, 16000
    with _vc.options(fe_fused=1):
        cases = _fe_refs(B, L, None, 6, seed=13)
        g1 = _FeGraph(B, L, None, cases[0])
        g2 = _FeGraph(B, L, None, cases[1])
        try:
            for k, case in enumerate(cases):
                fg = (g1, g2)[k % 2]
                _fe_check(fg.replay(case), case, None, 'graph %d replay %d' % (1 + k % 2, 1 + k // 2),
                          oracle=k < 2)
        finally:
            _free(g1.graph, g2.graph)


# --------------------------------------------------------------------------------------------- vocoder
def _amp_of_speech(L, seed, gain):
    y = fo.synth_speech(1, L, seed=seed)[0].astype(np.float64) * gain
    y = y[:80 * (len(y) // 80)]
    return np.abs(vo.stft(y, 400, 80, 400)).astype(np.float64)          # [bins, F]


@pytest.mark.parametrize('momentum', [0.0, 0.99])
def test_vocoder_graph_replay_with_trace(momentum):
    """griffin_lim_batch, 32 iterations, trace=True (the trace memset and the per-utterance atomicAdd into it); with
    momentum 0.99 also the state kept in the workspace.  Three replays with new magnitudes and phases: the waveform
    bit-identical to eager, the trace within 1e-5 relative of eager's; with momentum the replayed waveform is also held
    to test_vocoder_momentum_gpu.py's bound against tests/fgla_ref.py (3x the reference's own float32 / float64
    distance)."""
    import audio_lib
    B, n_iter = 3, 32
    rng = np.random.RandomState(4)
    cases = []
    for k in range(3):
        amps = [_amp_of_speech(8000, 50 + 7 * k + b, 0.1 * 3.0 ** ((k + b) % 3)) for b in range(B)]
        amp = np.stack([a.T for a in amps]).astype(np.float32)                  # [B, F, 201]
        ph = rng.uniform(0, np.pi, amp.shape).astype(np.float32)
        d_amp, d_ph = torch.from_numpy(amp).cuda(), torch.from_numpy(ph).cuda()
        w, t = audio_lib.griffin_lim_batch(d_amp, None, 400, 80, num_iters=n_iter, phase0=d_ph, trace=True,
                                           momentum=momentum)
        cases.append(dict(amps=amps, ph=ph, d_amp=d_amp, d_ph=d_ph, wav=w.clone(), tr=t.clone()))
    s_amp, s_ph = cases[0]['d_amp'].clone(), cases[0]['d_ph'].clone()
    g, (wav, tr) = _capture(lambda: audio_lib.griffin_lim_batch(s_amp, None, 400, 80, num_iters=n_iter, phase0=s_ph,
                                                                trace=True, momentum=momentum))
    try:
        for k in (1, 2, 0):
            c = cases[k]
            s_amp.copy_(c['d_amp'])
            s_ph.copy_(c['d_ph'])
            g.replay()
            torch.cuda.synchronize()
            _same(wav, c['wav'], 'replay of case %d: wav' % k)
            assert torch.isfinite(tr).all() and float(tr[1:].min()) > 0.0
            assert torch.allclose(tr, c['tr'], rtol=1e-5, atol=0.0), float(((tr - c['tr']) / c['tr']).abs().max())
            if momentum:
                b = k % B
                ph0 = c['ph'][b].T.astype(np.float64)
                r64 = fr.griffin_lim_momentum(c['amps'][b], 400, 80, n_iter, momentum, phase0=ph0)
                r32 = fr.griffin_lim_momentum(c['amps'][b], 400, 80, n_iter, momentum, phase0=ph0, dtype=np.float32)
                gap = fr.rel_l2(r32, r64)
                got = wav[b].cpu().numpy()
                assert 0.0 < gap and fr.rel_l2(got, r64) <= 3.0 * gap, (k, fr.rel_l2(got, r64), gap)
    finally:
        _free(g)


# --------------------------------------------------------------------------------------------- decoder
def _models(dtype):
    """bench.py's models: encoder (enc_14 weights) + decoder of the shipped sizes (seeded weights) sharing one store of
    `dtype`; for 'mxfp8' the decoder alone (it needs a store of its own) on posteriors."""
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    from oracle import model_oracle as mo
    dec_cfg = json.load(open(os.path.join(HP, 'decoder_cfg_d.json')))
    dec_cfg.update(is_training=False)
    with contextlib.redirect_stdout(io.StringIO()):
        if dtype == 'mxfp8':
            dec_cfg.update(compute_dtype='mxfp8')
            dec = decoder_specs(dec_cfg, None, None)
        else:
            enc_cfg = json.load(open(os.path.join(HP, 'encoder_cfg_d.json')))
            enc_cfg.update(is_training=False, compute_dtype=dtype, model_path=os.path.join(GOLDEN, 'enc_14_ckpt'))
            dec = decoder_specs(dec_cfg, None, encoder_spec_phn(enc_cfg, None))
    dec.store.load_dict(dict(mo.init_weights(dec_cfg, 'decoder', seed=2, perturb_bn=True)), strict=False)
    return dec


def _features(k):
    """64 windows of front-end features of 32 x 4 s of audio (the bench's step input), new audio for each k."""
    import audio_lib
    wav = torch.from_numpy(fo.synth_speech(32, 64000, seed=200 + k) * (0.05 * 3.0 ** (k % 3))).cuda()
    return audio_lib.calc_MFCC_input_batch(wav, None, out_frames=800, **FE_KW)[0].view(64, 400, 80).clone()


def _posteriors(k):
    rng = np.random.RandomState(300 + k)
    return torch.softmax(torch.from_numpy(rng.standard_normal((64, 400, 61)) * 3.0), -1).float().cuda()


DEC_KEYS = ('y_mel', 'y_stft', 'y_phn')


@pytest.mark.parametrize('dtype', ['bfloat16', 'mxfp8', 'float32'])
def test_decoder_forward_graph_replay(dtype):
    """dec.forward at 64 windows.  bfloat16: the encoder's fused front, the bank256 split-K tickets and gemm16;
    mxfp8: the MX-FP8 bank, the projections' split-K workspace and its reduce; float32: the gemm16 f16x3 path and the
    float32 GRU scratch.  Three replays, new inputs each, bit-identical to eager."""
    dec = _models(dtype)
    make = _posteriors if dtype == 'mxfp8' else _features
    xs = [make(k) for k in range(3)]
    refs = []
    for x in xs:
        o = dec.forward(x)
        refs.append({n: o[n].clone() for n in DEC_KEYS})
    s_x = xs[0].clone()
    g, out = _capture(lambda: dec.forward(s_x))
    try:
        for k in (1, 2, 0):
            s_x.copy_(xs[k])
            g.replay()
            torch.cuda.synchronize()
            for n in DEC_KEYS:
                _same(out[n], refs[k][n], '%s replay of input %d: %s' % (dtype, k, n))
            assert torch.isfinite(out['y_mel']).all() and torch.isfinite(out['y_stft']).all()
    finally:
        _free(g)


def test_bench_step_graph_replay():
    """bench.py's step in one graph: front-end (out_frames=800) on 32 x 4 s, view as 64 windows, encoder + decoder
    (bf16).  New audio for every replay; features and outputs bit-identical to the same step run eagerly."""
    import audio_lib
    dec = _models('bfloat16')
    B, L = 32, 64000
    wavs = [torch.from_numpy(fo.synth_speech(B, L, seed=400 + k) * np.float32(0.02 * 4.0 ** k)).cuda()
            for k in range(3)]

    def step(w):
        f = audio_lib.calc_MFCC_input_batch(w, None, out_frames=800, **FE_KW)
        o = dec.forward(f[0].view(2 * B, 400, 80))
        return f, o

    refs = []
    for w in wavs:
        f, o = step(w)
        refs.append(([t.clone() for t in f], {n: o[n].clone() for n in DEC_KEYS}))
    s_w = wavs[0].clone()
    g, (f, o) = _capture(lambda: step(s_w))
    try:
        for k in (1, 2, 0):
            s_w.copy_(wavs[k])
            g.replay()
            torch.cuda.synchronize()
            for name, a, b in zip(FE_NAMES, f, refs[k][0]):
                _same(a, b, 'step replay %d: front-end %s' % (k, name))
            for n in DEC_KEYS:
                _same(o[n], refs[k][1][n], 'step replay %d: %s' % (k, n))
    finally:
        _free(g)
