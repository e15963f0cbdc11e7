"""One plan, many calls: the front-end and vocoder plans are cached per configuration (audio_lib._get_plan,
_get_voc_plan), so every call of a process shares one.  A plan must be read-only after creation and every call's
scratch its own, so that
  * consecutive calls with different audio and batch sizes do not see each other's state, even when a call's fresh
    workspace starts out NaN-filled (a kernel that cleared its counters only after itself would read NaN words);
  * calls of one plan on two streams, with nothing ordering the streams against each other, compute what they compute
    alone.
The two-stream tests depend on how the launches of the two streams happen to overlap: on a library that shares a
plan's counters or a cached workspace between streams they can fail or pass by luck.  tests/test_graph_replay_gpu.py
holds the deterministic check of the front-end's counters."""
import numpy as np
import pytest
import torch

from conftest import FE_KW, poison_gpu_state
from oracle import frontend_oracle as fo

pytestmark = pytest.mark.gpu

FE_NAMES = ('mfcc', 'mel', 'pdb')
FORM_TOL = {'mfcc': 4e-6, 'mel': 2e-6, 'pdb': 2e-6}      # one launch vs two: test_graph_replay_gpu.py


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError('%s: not bit-identical: %d of %d values differ, max |diff| %.3e'
                             % (what, int((got != want).sum()), got.numel(), float(d.nan_to_num(float('inf')).max())))


def _fe_batch(B, L, seed):
    """Speech-like audio at a gain per utterance and ragged lengths (the shortest 1119 samples: one feature tile)."""
    wav = fo.synth_speech(B, L, seed=seed)
    lens = np.array([L - 97 * b if b % 3 else max(1119, L // (b + 2)) for b in range(B)], np.int32)
    for b in range(B):
        wav[b] *= np.float32(0.01 * 5.0 ** ((b + seed) % 3))
        wav[b, lens[b]:] = 0.0
    return torch.from_numpy(wav).cuda(), torch.from_numpy(lens).cuda()


def _fe(wav, lens):
    import audio_lib
    return tuple(t.clone() for t in audio_lib.calc_MFCC_input_batch(wav, lens, **FE_KW))


@pytest.mark.parametrize('fused', [1, 0])
def test_frontend_calls_with_changing_inputs_after_poisoning(fused):
    """Batches of 6, 32 and 3 utterances with different audio, called in turn (A B C A B C) after poison_gpu_state(),
    so that a call's fresh workspace holds NaN: every result equals the same call made alone (right after its own
    poisoning), and the one-launch form stays within FORM_TOL of the two-launch form."""
    import _vc
    batches = [_fe_batch(6, 16000, 1), _fe_batch(32, 64000, 2), _fe_batch(3, 8000, 3)]
    with _vc.options(fe_fused=fused):
        alone = []
        for w, n in batches:
            poison_gpu_state()
            alone.append(_fe(w, n))
        poison_gpu_state()
        for rep in range(2):
            for i, (w, n) in enumerate(batches):
                got = _fe(w, n)
                for name, a, b in zip(FE_NAMES, got, alone[i]):
                    _same(a, b, 'fe_fused=%d batch %d call %d: %s' % (fused, w.shape[0], rep + 1, name))
                    assert torch.isfinite(a).all()
    if fused:
        with _vc.options(fe_fused=0):
            for (w, n), a in zip(batches, alone):
                for name, x, y in zip(FE_NAMES, a, _fe(w, n)):
                    assert float((x - y).abs().max()) < FORM_TOL[name], (w.shape[0], name, float((x - y).abs().max()))


def _two_streams(calls):
    """Runs calls[i] on side stream i % 2, both streams ordered only behind the work already on the current stream
    (the uploads), none behind the other; returns the results once both streams are done."""
    main = torch.cuda.current_stream()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(main)
    out = []
    for i, fn in enumerate(calls):
        with torch.cuda.stream(streams[i % 2]):
            out.append(fn())
    for s in streams:
        main.wait_stream(s)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('fused', [1, 0])
def test_frontend_one_plan_on_two_streams(fused):
    """8 front-end calls of one plan (different audio each) alternating between two streams with no ordering between
    them: each result bit-identical to the same call alone on one stream."""
    import _vc
    import audio_lib
    batches = [_fe_batch(8, 32000, 10 + i) for i in range(8)]
    with _vc.options(fe_fused=fused):
        alone = [_fe(w, n) for w, n in batches]
        torch.cuda.synchronize()
        got = _two_streams([lambda w=w, n=n: audio_lib.calc_MFCC_input_batch(w, n, **FE_KW) for w, n in batches])
    for i, (g, a) in enumerate(zip(got, alone)):
        for name, x, y in zip(FE_NAMES, g, a):
            _same(x, y, 'fe_fused=%d call %d on stream %d: %s' % (fused, i, i % 2, name))


def test_vocoder_one_plan_on_two_streams():
    """8 griffin_lim_batch calls (momentum 0.99, trace=True: the momentum state and the trace scratch live in the
    workspace) alternating between two unordered streams: each waveform bit-identical to the same call alone, each
    trace within 1e-5 relative (its float atomicAdd has no fixed order)."""
    import audio_lib
    from oracle import vocoder_oracle as vo
    rng = np.random.RandomState(8)
    ins = []
    for i in range(8):
        amp = np.stack([np.abs(vo.stft(fo.synth_speech(1, 8000, seed=60 + 2 * i + b)[0].astype(np.float64)
                                       * (0.1 * 3.0 ** ((i + b) % 3)), 400, 80, 400)).T for b in range(2)])
        ph = rng.uniform(0, np.pi, amp.shape)
        ins.append((torch.from_numpy(amp.astype(np.float32)).cuda(), torch.from_numpy(ph.astype(np.float32)).cuda()))

    def call(a, p):
        return audio_lib.griffin_lim_batch(a, None, 400, 80, num_iters=16, phase0=p, trace=True, momentum=0.99)

    alone = [tuple(t.clone() for t in call(a, p)) for a, p in ins]
    torch.cuda.synchronize()
    got = _two_streams([lambda a=a, p=p: call(a, p) for a, p in ins])
    for i, ((w, t), (w0, t0)) in enumerate(zip(got, alone)):
        _same(w, w0, 'call %d on stream %d: wav' % (i, i % 2))
        assert torch.allclose(t, t0, rtol=1e-5, atol=0.0), (i, float(((t - t0) / t0).abs().nan_to_num(0.0).max()))
