"""GPU checks of the deterministic Griffin-Lim phase start (csrc/vc_spsi.hip through vc_phase_spsi, audio_lib.phase_spsi,
phase0='spsi', convert_batch(phase='spsi')) against the CPU reference tests/spsi_ref.py.

Every operation of the definition is an integer operation or one correctly rounded IEEE operation (float32 subtraction,
multiplication by 0.5 / 2, division; float64 multiplication; round-to-nearest-even conversions), so the device's phase
must equal the reference's bit for bit: arrays are compared as uint32 words, NaN frames and signed zeros included."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import fgla_ref as fr
import spsi_ref as sr
from test_conversion_gpu import _cfgs

pytestmark = pytest.mark.gpu

ALPHA = 0.99
CONFIGS = [(16, 4), (400, 80), (800, 40), (1024, 256)]            # n_fft / hop; 1024: 513 bins, above the block of 256
KINDS = ('voiced', 'noise', 'ints', 'gaps', 'ramps', 'edges', 'valley', 'nan', 'wild')


def _chunk():
    import audio_lib
    return audio_lib.SPSI_CHUNK_FRAMES


@functools.lru_cache(maxsize=None)
def _voiced(n_fft, hop):
    """[80, bins] float32 magnitudes of the synthetic voiced signal (computed once per transform size, never modified)."""
    a = np.ascontiguousarray(sr.voiced_magnitudes(80, n_fft, hop).T, dtype=np.float32)
    a.setflags(write=False)
    return a


def _magnitudes(kind, F, n_fft, hop, seed=0):
    """[F, bins] float32 of one kind."""
    nb = 1 + n_fft // 2
    rng = np.random.RandomState(1000 * seed + 17 * KINDS.index(kind) + F)
    v = _voiced(n_fft, hop)[:F].copy()
    t = np.arange(F)
    if kind == 'voiced':
        m = v
    elif kind == 'noise':                                          # nearly every other bin is a peak
        m = rng.rand(F, nb)
    elif kind == 'ints':                                           # ties, plateaus, unowned bins
        m = rng.randint(0, 4, (F, nb))
    elif kind == 'gaps':                                           # all-zero and all-equal frames between voiced ones
        m = v
        m[t % 5 == 1] = 0.0
        m[t % 5 == 3] = 1.0
    elif kind == 'ramps':                                          # no interior peak: the state carries through
        m = v
        up = np.arange(nb, dtype=np.float32)
        m[t % 3 == 1] = up
        m[t % 3 == 2] = up[::-1]
    elif kind == 'edges':                                          # single peaks at bin 1 and at nb-2
        m = np.zeros((F, nb))
        m[t % 2 == 0, 1] = 5.0
        m[t % 2 == 1, nb - 2] = 3.0
        m[:, 0] = 0.5
    elif kind == 'valley':                                         # two peaks sharing one valley bin
        m = np.zeros((F, nb))
        for f in range(F):
            k = 1 + f % (nb - 4)
            m[f, k:k + 3] = (3.0, 1.0, 2.0)
    elif kind == 'nan':                                            # whole frames of NaN between voiced ones
        m = v
        m[t % 4 == 1] = np.nan
    else:                                                          # outside the expected inputs: still defined, still in range
        m = v
        wild = rng.rand(F, nb)
        m[wild < 0.02] = np.nan
        m[(wild >= 0.02) & (wild < 0.04)] = np.inf
        m[(wild >= 0.04) & (wild < 0.06)] = -np.inf
        m[(wild >= 0.06) & (wild < 0.10)] *= -1.0
    return np.ascontiguousarray(m, dtype=np.float32)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ref_batch(amp, n_frames, n_fft, hop):
    return np.stack([sr.phase_sequential(amp[b], n_fft, hop, None if n_frames is None else n_frames[b])
                     for b in range(amp.shape[0])])


@pytest.mark.parametrize('n_fft,hop', CONFIGS)
@pytest.mark.parametrize('rel', ['1', '2', 'C-1', 'C', 'C+1', '2C+1'])
def test_bit_exact_at_every_frame_count(n_fft, hop, rel):
    """One utterance per kind of magnitudes, n_frames=None, Fmax = F around the chunk length C."""
    import audio_lib
    C = _chunk()
    F = {'1': 1, '2': 2, 'C-1': C - 1, 'C': C, 'C+1': C + 1, '2C+1': 2 * C + 1}[rel]
    amp = np.stack([_magnitudes(k, F, n_fft, hop) for k in KINDS])
    d_amp = torch.from_numpy(amp).cuda()
    got = audio_lib.phase_spsi(d_amp, None, hop, n_fft)
    assert got.shape == d_amp.shape and got.dtype == torch.float32 and got.is_cuda
    want = _ref_batch(amp, None, n_fft, hop)
    bad = [KINDS[b] for b in range(len(KINDS)) if not np.array_equal(_bits(got[b]), _bits(want[b]))]
    assert not bad, bad
    assert np.array_equal(_bits(d_amp), _bits(amp))                # the input is only read


@pytest.mark.parametrize('n_fft,hop', CONFIGS)
def test_ragged_batch_zero_rows_and_batch_independence(n_fft, hop):
    """n_frames = (0, 1, 2C+1) inside Fmax = 2C+3 for every kind; garbage beyond n_frames must not leak in; the rows
    beyond are exactly +0.0; the long utterance alone at Fmax = 2C+1 gives the same bits."""
    import audio_lib
    C = _chunk()
    Fmax, nf3 = 2 * C + 3, (0, 1, 2 * C + 1)
    amp = np.stack([_magnitudes(k, Fmax, n_fft, hop, seed=1 + j) for k in KINDS for j in range(3)])
    nf = list(nf3) * len(KINDS)
    for b, n in enumerate(nf):
        amp[b, n:] = np.float32(7.5) + amp[b, n:][::-1]            # what lies beyond an utterance is not its business
    d_amp = torch.from_numpy(amp).cuda()
    out = torch.full(d_amp.shape, float('nan'), device='cuda')
    got = audio_lib.phase_spsi(d_amp, nf, hop, n_fft, out=out)
    assert got is out
    want = _ref_batch(amp, nf, n_fft, hop)
    g = _bits(got)
    for b, n in enumerate(nf):
        assert np.array_equal(g[b], _bits(want[b])), (KINDS[b // 3], n)
        assert not g[b, n:].any()                                  # +0.0 bit for bit
    assert np.array_equal(_bits(d_amp), _bits(amp))
    # n_frames as a device tensor; an utterance alone, at another Fmax
    again = audio_lib.phase_spsi(d_amp, torch.tensor(nf, dtype=torch.int32, device='cuda'), hop, n_fft)
    assert np.array_equal(_bits(again), g)
    for k in range(len(KINDS)):
        b = 3 * k + 2
        alone = audio_lib.phase_spsi(d_amp[b:b + 1, :2 * C + 1].contiguous(), None, hop, n_fft)
        assert np.array_equal(_bits(alone[0]), g[b, :2 * C + 1]), KINDS[k]


def _power_to_amp(P, nf):
    import _vc
    import audio_lib
    B, F, nb = P.shape
    d_nf = None if nf is None else torch.tensor(nf, dtype=torch.int32, device='cuda')
    amp = torch.empty_like(P)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(P), _vc.ptr(d_nf), B, F, nb, 0.01, 1.0, _vc.ptr(amp), _vc.current_stream()))
    return amp


@pytest.mark.parametrize('n_fft,hop', [(400, 80), (800, 40)])
def test_vocoder_takes_the_spsi_phase(n_fft, hop):
    import audio_lib
    F, nf = 70, [70, 41]
    amp = np.stack([_magnitudes('voiced', F, n_fft, hop), _magnitudes('noise', F, n_fft, hop)])
    d_amp = torch.from_numpy(amp).cuda()
    ph = audio_lib.phase_spsi(d_amp, nf, hop, n_fft)
    for m in (0.0, ALPHA):
        got = audio_lib.griffin_lim_batch(d_amp, nf, n_fft, hop, num_iters=3, phase0='spsi', momentum=m, seed=5, utt_ids=[8, 9])
        want = audio_lib.griffin_lim_batch(d_amp, nf, n_fft, hop, num_iters=3, phase0=ph, momentum=m)
        assert torch.equal(got, want) and torch.isfinite(got).all()
    assert not torch.equal(got, audio_lib.griffin_lim_batch(d_amp, nf, n_fft, hop, num_iters=3, phase0='device', momentum=ALPHA))
    # through the power-spectrum driver
    P = torch.from_numpy(np.random.RandomState(2).uniform(0.0, 0.9, amp.shape).astype(np.float32)).cuda()
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=hop, win_length=n_fft, mean_abs_amp_norm=0.045, n_iter=3,
              momentum=ALPHA)
    ph = audio_lib.phase_spsi(_power_to_amp(P, nf), nf, hop, n_fft)
    assert torch.equal(audio_lib.from_power_to_wav_batch(P, nf, phase0='spsi', **kw),
                       audio_lib.from_power_to_wav_batch(P, nf, phase0=ph, **kw))
    with pytest.raises(ValueError, match="'spsi'"):
        audio_lib.griffin_lim_batch(d_amp, nf, n_fft, hop, phase0='nope')


def test_graph_replay_equals_eager():
    """One capture of griffin_lim_batch(phase0='spsi', num_iters=3): a linear chain on one stream."""
    import audio_lib
    amp = torch.from_numpy(np.stack([_magnitudes('voiced', 70, 400, 80), _magnitudes('ints', 70, 400, 80)])).cuda()
    fn = lambda: audio_lib.griffin_lim_batch(amp, None, 400, 80, num_iters=3, phase0='spsi', momentum=ALPHA)
    eager = fn().clone()
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
    for _ in range(2):
        out.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    del g


def test_convergence_from_the_spsi_start():
    """The synthetic voiced signal at 400 / 80, 200 frames, momentum 0.99, num_iters 9 (8 projections): the device's
    spectral convergence agrees with the float64 reference's within 3x the reference's own float32-to-float64 distance
    (the bound of tests/test_vocoder_momentum_gpu.py), and lies below the device's own from a random ('device') start."""
    import audio_lib
    a64 = sr.voiced_magnitudes(200, 400, 80)                        # [bins, F]
    a32 = np.ascontiguousarray(a64.T, dtype=np.float32)
    ph = sr.phase_sequential(a32, 400, 80).T.astype(np.float64)
    r64 = fr.griffin_lim_momentum(a64, 400, 80, 9, ALPHA, phase0=ph)
    r32 = fr.griffin_lim_momentum(a64, 400, 80, 9, ALPHA, phase0=ph, dtype=np.float32)
    gap = fr.rel_l2(r32, r64)
    sc_ref = fr.sc(r64, a64, 400, 80)
    d_amp = torch.from_numpy(a32)[None].cuda()
    kw = dict(num_iters=9, momentum=ALPHA)
    got = audio_lib.griffin_lim_batch(d_amp, None, 400, 80, phase0='spsi', **kw)[0].cpu().numpy()
    rnd = audio_lib.griffin_lim_batch(d_amp, None, 400, 80, phase0='device', seed=0, **kw)[0].cpu().numpy()
    sc_got, sc_rnd = fr.sc(got, a64, 400, 80), fr.sc(rnd, a64, 400, 80)
    print('SC spsi: device %.5f reference %.5f (waveform rel L2 %.3e, float32 gap %.3e); device random start %.5f'
          % (sc_got, sc_ref, fr.rel_l2(got, r64), gap, sc_rnd))
    assert 0.0 < gap and fr.rel_l2(got, r64) <= 3.0 * gap
    assert abs(sc_got - sc_ref) <= 3.0 * gap * sc_ref
    assert sc_got < sc_rnd


# --------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def f32_models(golden_dir):
    """The decoder configuration of tests/test_convert_batch_gpu.py."""
    from oracle import model_oracle as mo
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    enc_cfg, dec_cfg, c = _cfgs(golden_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
        dec = decoder_specs(dec_cfg, None, enc)
    dec.store.load_dict(dict(mo.init_weights(dec_cfg, 'decoder', seed=2, perturb_bn=True)), strict=False)
    return dec, c


def test_spsi_phase_through_convert_batch(f32_models):
    import audio_lib
    import conversion
    from oracle import frontend_oracle as fo
    dec, c = f32_models
    lens = [24000, 17000]                                           # 1.5 s and 1.06 s: one window of 400 frames each
    wav = np.zeros((2, max(lens)), np.float32)
    for b, L in enumerate(lens):
        wav[b, :L] = fo.synth_speech(1, L, seed=21 + b)[0]
    d_wav = torch.from_numpy(wav).cuda()
    N = 4
    conversion.convert_batch(dec, d_wav, lens, c, n_iter=N, phase='spsi', giffin_lim_input=True, momentum=ALPHA)    # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = conversion.convert_batch(dec, d_wav, lens, c, n_iter=N, phase='spsi', giffin_lim_input=True, momentum=ALPHA)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert r.n_frames == [400, 400] and torch.isfinite(r.y_wav_pred).all() and torch.isfinite(r.y_wav_true).all()
    # the predicted spectrum starts from the phase of its own magnitudes
    ph = audio_lib.phase_spsi(_power_to_amp(r.stft_pred, r.n_frames), r.n_frames, 80, 400)
    r2 = conversion.convert_batch(dec, d_wav, lens, c, n_iter=N, phase=ph, momentum=ALPHA)
    assert torch.equal(r2.stft_pred, r.stft_pred) and torch.equal(r2.y_wav_pred, r.y_wav_pred)
    # and the true spectrum from its own
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80, win_length=400, mean_abs_amp_norm=15 * 0.003, n_iter=N,
              momentum=ALPHA)
    assert torch.equal(r.y_wav_true, audio_lib.from_power_to_wav_batch(r.stft_true, r.n_frames, phase0='spsi', **kw))
    assert not torch.equal(r.y_wav_true, audio_lib.from_power_to_wav_batch(r.stft_true, r.n_frames, phase0=ph, **kw))
    # seed and utt_ids are ignored
    r3 = conversion.convert_batch(dec, d_wav, lens, c, n_iter=N, phase='spsi', momentum=ALPHA, seed=123, utt_ids=[7, 9])
    assert torch.equal(r3.y_wav_pred, r.y_wav_pred)
