"""evaluation.py on the device against tests/mcd_ref.py: exact integer cases (totals, lengths and whole paths equal),
speech-like ragged pairs from 1 x 1 to 3,000 x 3,700 frames (path validity, the derived float32 bound, the float32
restatement as a regression yardstick), score mode against path mode, alone against batched, graph replay, the band,
the frame-synchronous mean, the cepstra, no host synchronisation, convert_batch's outputs end to end, gain, and an
utterance against its own 48 kHz copy."""
import numpy as np
import pytest
import torch

import mcd_ref as mr
from oracle import frontend_oracle as fo
from test_conversion_gpu import _fe_kwargs
from test_convert_batch_gpu import _dev, _ragged, f32_models                         # noqa: F401 (fixture)
from test_mcd_cpu import CFG

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _np(t):
    return t.cpu().numpy()


def _pad(rows):
    n = max(len(r) for r in rows)
    out = np.zeros((len(rows), n) + rows[0].shape[1:], np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _paths(res, b):
    n = int(res.path_len[b])
    p = _np(res.path[b])
    assert (p[n:] == -1).all()
    return p[:n]


# --------------------------------------------------------------------------------------------- 1. exact cases
def _int_frames(rng, F, hi=4):
    return (rng.randint(0, hi, (F, 1)) * np.ones((1, 8))).astype(np.float32)      # d = 4 |delta|: every cost an integer


def test_exact_integer_cases_equal_the_reference():
    import evaluation as ev
    rng = np.random.RandomState(3)
    a0 = (np.arange(300)[:, None] % 7 * np.ones((1, 8))).astype(np.float32)
    pairs = [(a0, a0), (a0[:90], np.repeat(a0[:90], 3, axis=0)), (_int_frames(rng, 1), _int_frames(rng, 1)),
             (_int_frames(rng, 1), _int_frames(rng, 40)), (_int_frames(rng, 33), _int_frames(rng, 1)),
             (_int_frames(rng, 257), _int_frames(rng, 300)), (_int_frames(rng, 1025), _int_frames(rng, 513)),
             (_int_frames(rng, 2100, 3), _int_frames(rng, 1500, 3))]
    la, lb = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    ca, cb = _pad([a for a, _ in pairs]), _pad([b for _, b in pairs])
    for band in (None, 40):
        res = ev.dtw_batch(ca, cb, la, lb, band=band, return_path=True, scale=1.0)
        for b, (x, y) in enumerate(pairs):
            total, n, path = mr.dtw(x, y, 1.0, band)
            assert float(res.total[b]) == total and int(res.path_len[b]) == n, (b, band, float(res.total[b]), total, int(res.path_len[b]), n)
            assert float(res.mcd[b]) == np.float32(np.float32(total) / np.float32(n))
            assert np.array_equal(_paths(res, b), path), (b, band)
    res = ev.dtw_batch(ca[:2], cb[:2], la[:2], lb[:2], return_path=True)
    assert _np(res.total).tolist() == [0.0, 0.0] and _np(res.path_len).tolist() == [300, 270]
    assert np.array_equal(_paths(res, 0), np.stack([np.arange(300)] * 2, 1))


# --------------------------------------------------------------------------------------------- 2.-4., 6. real-valued cases
SHAPES = [(1, 1), (1, 50), (37, 1), (600, 700), (1500, 1300), (3000, 3700)]


@pytest.fixture(scope='module')
def speech_pairs():
    """Speech-like mel from the device front-end; side b is side a's waveform resampled (linear interpolation) to
    0.8x - 1.25x its length.  Returns the device's own float32 cepstra (padded) and the lengths."""
    import audio_lib
    import evaluation as ev
    kw = _fe_kwargs(CFG)
    mels_a, mels_b = [], []
    for k, (Fa, Fb) in enumerate(SHAPES):
        La, Lb = max(80 * (Fa - 1) + 1, 401), max(80 * (Fb - 1) + 1, 401)
        wa = fo.synth_speech(1, La, seed=20 + k)[0]
        wb = np.interp(np.linspace(0, La - 1, Lb), np.arange(La), wa).astype(np.float32)
        for w, F, dst in ((wa, Fa, mels_a), (wb, Fb, mels_b)):
            mel = audio_lib.calc_MFCC_input_batch(np.ascontiguousarray(w).reshape(1, -1), None, **kw)[1]
            dst.append(_np(mel[0])[:F])
    la, lb = [s[0] for s in SHAPES], [s[1] for s in SHAPES]
    mel_a, mel_b = _dev(_pad(mels_a)), _dev(_pad(mels_b))
    ca, cb = ev.mel_cepstra(mel_a), ev.mel_cepstra(mel_b)
    return dict(mel_a=mel_a, mel_b=mel_b, ca=ca, cb=cb, la=la, lb=lb, ca_h=_np(ca), cb_h=_np(cb))


@pytest.fixture(scope='module')
def references(speech_pairs):
    """Float64 optimum and the float32 restatement on the device's own cepstra, unbanded and with a narrow band."""
    s = speech_pairs
    out = {}
    for band in (None, 30):
        for b, (Fa, Fb) in enumerate(SHAPES):
            x, y = s['ca_h'][b, :Fa], s['cb_h'][b, :Fb]
            t64, n64, _ = mr.dtw(x, y, 25.0, band, np.float64, want_path=False)
            t32, n32, _ = mr.dtw(x, y, 25.0, band, np.float32, want_path=False)
            out[(band, b)] = (float(t64), n64, float(t32), n32)
    return out


def _check_real(s, res, refs, band):
    worst = 0.0
    for b, (Fa, Fb) in enumerate(SHAPES):
        x, y = s['ca_h'][b, :Fa], s['cb_h'][b, :Fb]
        t64, n64, t32, n32 = refs[(band, b)]
        total = float(res.total[b])
        path = _paths(res, b)
        mr.check_path(path, Fa, Fb, band)                                          # (a)
        assert len(path) == int(res.path_len[b])
        bound = 2.0 * (Fa + Fb + 24 + 2) * EPS
        cost = mr.path_cost(x, y, path, 25.0)
        gap = (cost - t64) / t64 if t64 > 0 else cost - t64
        own = abs(total - cost) / cost if cost > 0 else abs(total - cost)
        err = abs(total - t64) / t64 if t64 > 0 else abs(total - t64)
        yard = abs(t32 - t64) / t64 if t64 > 0 else abs(t32 - t64)
        ulp = float(np.spacing(np.float32(total))) / total if total > 0 else 0.0
        print('band %s  %5d x %5d: path gap %.3e (bound %.3e)  total vs own path %.3e (bound %.3e)  total err %.3e  float32 '
              'restatement %.3e  ratio %.2f' % (band, Fa, Fb, gap, bound, own, bound / 2, err, yard, err / max(yard, ulp, 1e-300)))
        assert gap <= bound, (b, gap, bound)                                       # (b)
        assert own <= bound / 2, (b, own, bound)                                   # (c)
        assert err <= 3.0 * (yard if yard > 0 else ulp), (b, err, yard, ulp)       # (d)
        worst = max(worst, err / max(yard, ulp, 1e-300))
        assert float(res.mcd[b]) == np.float32(np.float32(total) / np.float32(len(path)))
    return worst


def test_speech_like_pairs_against_the_float64_optimum(speech_pairs, references):
    import evaluation as ev
    s = speech_pairs
    res = ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb'], return_path=True, scale=25.0)
    _check_real(s, res, references, None)
    # 3. score mode is bit-identical to path mode; 4. twice in a row and alone against inside the batch
    score = ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb'], scale=25.0)
    again = ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb'], scale=25.0)
    for k in ('total', 'path_len', 'mcd'):
        assert torch.equal(getattr(score, k), getattr(res, k)) and torch.equal(getattr(score, k), getattr(again, k)), k
    assert score.path is None
    for b in (0, 2, 3, 5):
        Fa, Fb = SHAPES[b]
        one = ev.dtw_batch(s['ca'][b:b + 1, :Fa].contiguous(), s['cb'][b:b + 1, :Fb].contiguous(), [Fa], [Fb], scale=25.0,
                           return_path=(b == 3))
        assert torch.equal(one.total, score.total[b:b + 1]) and torch.equal(one.path_len, score.path_len[b:b + 1]), b
        if b == 3:
            assert np.array_equal(_paths(one, 0), _paths(res, b))
    # mcd_batch on the mel tensors is the same thing
    m = ev.mcd_batch(s['mel_a'], s['mel_b'], s['la'], s['lb'], CFG)
    assert torch.equal(m.total, score.total) and torch.equal(m.mcd, score.mcd)


def test_band(speech_pairs, references):
    import evaluation as ev
    s = speech_pairs
    free = ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb'], return_path=True, scale=25.0)
    # the widest excursion of the unbanded optimum from the straight line, in frames of the longer side
    need = 0
    for b, (Fa, Fb) in enumerate(SHAPES):
        p = _paths(free, b).astype(np.int64)
        v = np.abs(p[:, 1] * (Fa - 1) - p[:, 0] * (Fb - 1)).max()
        need = max(need, -(-int(v) // max(Fa - 1, Fb - 1, 1)))
    wide = ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb'], band=need, return_path=True, scale=25.0)
    assert torch.equal(wide.total, free.total) and torch.equal(wide.path_len, free.path_len) and torch.equal(wide.path, free.path)
    narrow = ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb'], band=30, return_path=True, scale=25.0)
    _check_real(s, narrow, references, 30)
    assert (_np(narrow.total) >= _np(free.total)).all()


# --------------------------------------------------------------------------------------------- 5. graph
def test_graph_replay_with_new_contents_and_lengths(speech_pairs):
    """What mcd_batch launches -- cepstra of both sides, DTW with its back-track, the frame-synchronous mean -- captured
    on static mel buffers with the lengths in device tensors, then replayed after other mel and other lengths were
    copied into the same buffers: equal to the eager public call.  (mcd_batch itself takes host lengths and uploads them
    inside the call, so a capture of the public function would freeze its lengths; a caller who wants to replay with new
    lengths keeps them on the device as here.)  The first call is made outside the capture: it sets the kernel's LDS
    attribute."""
    import evaluation as ev
    s = speech_pairs
    mel_a, mel_b = s['mel_a'][2:5].clone(), s['mel_b'][2:5].clone()
    la = torch.tensor(s['la'][2:5], dtype=torch.int32, device='cuda')
    lb = torch.tensor(s['lb'][2:5], dtype=torch.int32, device='cuda')

    def launches():
        ca, cb = ev._cepstra_launch(mel_a, 24, 1), ev._cepstra_launch(mel_b, 24, 1)
        return ev._dtw_launch(ca, cb, la, lb, 25.0, -1, True), ev._frame_launch(ca, cb, la, lb, 25.0)

    launches()                                                                      # warm-up: code objects, attributes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out, out_f = launches()

    def check(len_a, len_b):
        g.replay()
        torch.cuda.synchronize()
        want = ev.mcd_batch(mel_a, mel_b, len_a, len_b, CFG, return_path=True)
        for k in ('total', 'path_len', 'mcd', 'path'):
            assert torch.equal(getattr(out, k), getattr(want, k)), k
        assert torch.equal(out_f.mcd, ev.mcd_batch(mel_a, mel_b, len_a, len_b, CFG, align='frame').mcd)

    check(s['la'][2:5], s['lb'][2:5])
    mel_a.copy_(torch.flip(s['mel_a'][2:5], dims=[0]) * 0.5)
    mel_b.copy_(s['mel_b'][2:5] + 0.01)
    new_a, new_b = [1200, 37, 5], [900, 1300, 1]
    la.copy_(torch.tensor(new_a, dtype=torch.int32))
    lb.copy_(torch.tensor(new_b, dtype=torch.int32))
    check(new_a, new_b)


# --------------------------------------------------------------------------------------------- 7., 8. frame mode, cepstra
def test_frame_synchronous_mean(speech_pairs):
    import evaluation as ev
    s = speech_pairs
    got = _np(ev.mcd_batch(s['mel_a'], s['mel_b'], s['la'], s['lb'], CFG, align='frame').mcd)
    for b, (Fa, Fb) in enumerate(SHAPES):
        x, y = s['ca_h'][b, :Fa], s['cb_h'][b, :Fb]
        want = mr.frame_mcd(x, y, 25.0)
        den = want if want > 0 else 1.0                                            # (the 1 x 1 pair's two frames are equal)
        yard = abs(float(mr.frame_mcd(x, y, 25.0, np.float32)) - want) / den
        err = abs(float(got[b]) - want) / den
        ulp = float(np.spacing(np.float32(want))) / den
        print('frame %5d x %5d: device %.3e  float32 restatement %.3e' % (Fa, Fb, err, yard))
        assert err <= 3.0 * max(yard, ulp), (b, err, yard)


def test_cepstra_against_the_float64_product(speech_pairs):
    import evaluation as ev
    s = speech_pairs
    mel = _np(s['mel_a'])
    tab = ev.dct_rows(80, 24, 1)
    want = mr.cepstra(mel, table=tab)
    m32 = mel.astype(np.float32)
    acc = np.zeros(want.shape, np.float32)
    for m in range(80):                                                             # the float32 restatement: one chain per output
        acc = acc + m32[..., m:m + 1] * tab[None, None, :, m]
    peak = np.abs(want).max()
    yard = np.abs(acc - want).max() / peak
    err = np.abs(s['ca_h'] - want).max() / peak
    print('cepstra: device %.3e  float32 restatement %.3e of peak' % (err, yard))
    assert err <= 3.0 * yard
    other = _np(ev.mel_cepstra(s['mel_a'], 13, 0))
    assert np.abs(other - mr.cepstra(mel, 13, 0)).max() <= 3.0 * yard * np.abs(other).max()
    # bf16 input equals float32 input after the same rounding
    bf = s['mel_a'].to(torch.bfloat16)
    assert torch.equal(ev.mel_cepstra(bf), ev.mel_cepstra(bf.float()))
    r1 = ev.mcd_batch(bf, s['mel_b'].to(torch.bfloat16), s['la'], s['lb'], CFG, align='frame')
    r2 = ev.mcd_batch(bf.float(), s['mel_b'].to(torch.bfloat16).float(), s['la'], s['lb'], CFG, align='frame')
    assert torch.equal(r1.mcd, r2.mcd)


# --------------------------------------------------------------------------------------------- 9. no host synchronisation
def test_no_host_synchronisation_inside_the_calls(speech_pairs):
    import evaluation as ev
    s = speech_pairs
    wav, lens = _ragged()
    d_wav = _dev(wav)
    d_48 = _dev(np.repeat(wav, 3, axis=1))
    lens48 = [3 * n for n in lens]
    calls = (lambda: ev.mcd_batch(s['mel_a'], s['mel_b'], s['la'], s['lb'], CFG, return_path=True),
             lambda: ev.mcd_batch(s['mel_a'], s['mel_b'], s['la'], s['lb'], CFG, align='frame'),
             lambda: ev.mcd_wav_batch(d_wav, lens, d_48, lens48, CFG, wav_sr_b=48000, band=100),
             lambda: ev.dtw_batch(s['ca'], s['cb'], s['la'], s['lb']))
    for c in calls:                                                                 # warm-up
        c()
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(o.mcd).all() for o in outs)


# --------------------------------------------------------------------------------------------- 10. end to end
def test_convert_batch_outputs_and_gain_invariance(f32_models):
    import conversion
    import evaluation as ev
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_batch(dec, wav, lens, c, vocode=False)
    got = _np(ev.mcd_batch(r.mel_pred, r.mel_true, r.n_frames, r.n_frames, c, align='frame').mcd)
    scale = mr.default_scale(c['M_dB_norm_factor'])
    ca, cb = _np(ev.mel_cepstra(r.mel_pred)), _np(ev.mel_cepstra(r.mel_true))     # the device's own cepstra, as in item 7
    for b, F in enumerate(r.n_frames):
        x, y = ca[b, :F], cb[b, :F]
        want = mr.frame_mcd(x, y, scale)
        yard = abs(float(mr.frame_mcd(x, y, scale, np.float32)) - want) / want
        err = abs(float(got[b]) - want) / want
        ulp = float(np.spacing(np.float32(want))) / want
        print('convert_batch utterance %d: frame MCD %.4f dB, host %.4f dB; device %.3e, float32 restatement %.3e'
              % (b, got[b], want, err, yard))
        assert err <= 3.0 * max(yard, ulp)
    dtw = ev.mcd_batch(r.mel_pred, r.mel_true, r.n_frames, r.n_frames, c)
    assert (_np(dtw.mcd) <= got * (1 + 1e-6)).all() and (_np(dtw.path_len) >= np.array(r.n_frames)).all()
    # gain: the front-end normalises the amplitude, and what is left of a gain moves c0 alone.  The front-end agrees with
    # its oracle to 2e-4 per mel value (smoke()); two sides, 80 bands, orthonormal rows: 25 * sqrt(2 * 80) * 2 * 2e-4 dB.
    g = ev.mcd_wav_batch(wav, lens, 0.5 * wav, lens, c)
    print('gain 0.5: MCD', _np(g.mcd))
    assert (_np(g.mcd) <= 25.0 * np.sqrt(2 * 80.0) * 2 * 2e-4).all()
    assert _np(g.path_len).tolist() == [1 + n // 80 for n in lens]


def test_an_utterance_against_its_own_48_khz_copy():
    """mcd_wav_batch(x at 16 kHz, the same x at 48 kHz): side b goes 16 -> 48 -> 16 kHz.  The bound comes from the
    resampler's round-trip error, not from this code.  The signal is the one of
    test_resample_gpu.test_round_trip_of_a_band_limited_signal (nothing above 6 kHz, Hann envelope), for which that test
    guarantees |round trip - x| <= eps * peak with eps = 3 x 1.683e-8 (the device measured 3.157e-8).

    Carried to decibels.  With s = mean_abs_amp_norm / mean|x| the front-end scales, pre-emphasises (gain <= 1 + 0.97) and
    windows (Hann, sum 200): every STFT bin of the error is at most dX = 200 * 1.97 * s * eps * peak.  A mel amplitude is
    the weighted 2-norm of the bins, A_m = ||sqrt(W_m) X||, so it moves by at most dA = sqrt(max_m sum_k W_mk) * dX.
    The mel dB is 40 log10(A) (amplitude_to_db of a power, reference audio_lib.py:172) floored at 80 dB below the
    utterance's maximum, i.e. at A_floor = A_max / 100, and every later step (the floor itself, the clip) is 1-Lipschitz,
    so a cell moves by at most ddB = (40 / ln 10) * dA / (A_floor - dA).  The changed scale factor s and the shift by the
    minimum are the same in every band: c0 only.  mel = M_dB_norm_factor * dB, the DCT rows are orthonormal, 80 bands:
    d(i, i) <= scale * sqrt(2 * 80) * M_dB_norm_factor * ddB.  Both sides have the same number of frames, the DTW total
    is at most the diagonal's and its path at least as long, so mcd <= max_i d(i, i).  On top of that the float32
    front-end sees two inputs that differ in their last bits; its tolerance against its oracle is 2e-4 per mel value
    (smoke()), on two sides: 25 * sqrt(2 * 80) * 2 * 2e-4 dB, the term of the gain test."""
    import audio_lib
    import evaluation as ev
    from scipy import signal
    n = 8000
    t = np.arange(n) / 16000.0
    rng = np.random.RandomState(2)
    x = sum(rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28)) for f in (110.0, 440.0, 1234.5, 3300.0, 5900.0))
    x = (x * np.hanning(n) / np.abs(x).max()).astype(np.float32)
    eps = 3 * 1.683e-8
    s = CFG['mean_abs_amp_norm'] / np.abs(x).mean()
    spec = np.abs(fo.stft(signal.lfilter([1, -CFG['pre_emphasis']], [1], s * x.astype(np.float64)), 400, 80, 400, 'hann'))
    W = fo.mel_filterbank(16000, 400, 80)
    a_max = np.sqrt(W @ spec.astype(np.float64) ** 2).max()
    dA = np.sqrt(W.sum(1).max()) * 200.0 * (1.0 + CFG['pre_emphasis']) * s * eps * np.abs(x).max()
    ddB = 40.0 / np.log(10.0) * dA / (a_max / 100.0 - dA)
    bound = 25.0 * np.sqrt(2 * 80.0) * (CFG['M_dB_norm_factor'] * ddB + 2 * 2e-4)
    up, n_up = audio_lib.resample_batch(_dev(x.reshape(1, -1)), None, sr_in=16000, sr_out=48000)
    assert list(n_up) == [3 * n]
    r = ev.mcd_wav_batch(x.reshape(1, -1), [n], up, [3 * n], CFG, wav_sr_b=48000)
    f = ev.mcd_wav_batch(x.reshape(1, -1), [n], up, [3 * n], CFG, wav_sr_b=48000, align='frame')
    print('16 kHz against its own 48 kHz copy: MCD %.3e dB (DTW), %.3e dB (frame); bound %.3e dB, of which the round trip %.3e'
          % (float(r.mcd[0]), float(f.mcd[0]), bound, 25.0 * np.sqrt(160.0) * CFG['M_dB_norm_factor'] * ddB))
    assert int(r.path_len[0]) >= 1 + n // 80
    assert float(r.mcd[0]) <= bound and float(f.mcd[0]) <= bound
