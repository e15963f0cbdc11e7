"""Dereverberation without a GPU: the argument checks of every new Python entry point and of the three launches (all made
before the device is touched), enhance.wpe_defaults, the properties of the restatement tests/dereverb_ref.py that the
device tests rely on, and the method's own figures on the committed room corpus."""
import ctypes as C

import numpy as np
import pytest

import dereverb_cases as dc
import dereverb_ref as ref

CFG_D = dict(hop_length=80, win_length=400, n_fft=None, sample_rate=16000)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------ arguments
def test_wpe_defaults_carry_delay_and_taps_to_the_hop():
    import enhance
    assert enhance.wpe_defaults(80, 16000, 400) == (16, 5) == ref.defaults(80, 16000, 400)
    assert enhance.wpe_defaults(128, 16000, 512) == (10, 4)           # nara_wpe's own framing: 10 taps; the delay is a window
    assert enhance.wpe_defaults(81, 16000, 400) == (16, 5) and enhance.wpe_defaults(80, 16000, 401) == (16, 6)
    assert enhance.wpe_defaults(1, 16000, 400) == (32, 64)            # clamped to the launch's limits
    assert enhance.wpe_defaults(4000, 16000, 400) == (1, 1)
    assert enhance.wpe_defaults(80, 16000, 400, span_ms=40.0) == (8, 5)
    for bad in ((0, 16000, 400), (80, -1, 400), (80, 16000, True), (80, 16000, 400, float('nan')), ('80', 16000, 400)):
        with pytest.raises(ValueError, match='wpe_defaults'):
            enhance.wpe_defaults(*bad)


def test_wpe_cfg_is_checked_on_the_host():
    import enhance
    c = enhance.wpe_cfg('t')
    assert (c.taps, c.delay, c.iterations, c.context) == (16, 5, 3, 1)
    assert c.floor_rel == np.float32(1e-6) and c.load_rel == np.float32(1e-8)
    c = enhance.wpe_cfg('t', taps=32, delay=64, iterations=16, context=8, floor_db=0.0, load=1.0)
    assert (c.taps, c.delay, c.iterations, c.context, c.floor_rel, c.load_rel) == (32, 64, 16, 8, 1.0, 1.0)
    assert enhance.wpe_cfg('t', hop_length=128, sr=16000, win_length=512).taps == 10
    for kw in (dict(taps=0), dict(taps=33), dict(taps=2.0), dict(taps=True), dict(delay=0), dict(delay=65), dict(iterations=0),
               dict(iterations=17), dict(context=-1), dict(context=9), dict(floor_db=1.0), dict(floor_db=-201.0),
               dict(floor_db=float('nan')), dict(load=-1e-9), dict(load=1.5), dict(load='x')):
        with pytest.raises(ValueError, match='t: '):
            enhance.wpe_cfg('t', **kw)
    with pytest.raises(ValueError, match='unknown dereverberation keyword'):
        enhance.check_wpe_keywords('t', dict(tap=3), 80, 16000, 400)
    cfg, rt = enhance.check_wpe_keywords('t', dict(taps=3, return_taps=True), 80, 16000, 400)
    assert cfg.taps == 3 and cfg.delay == 5 and rt is True


def test_frame_cap_is_exported_documented_and_at_least_20_seconds():
    import _vc
    import enhance
    lib = _vc.lib()
    for K in range(1, 33):
        assert lib.vc_wpe_max_frames(K) == ref.max_frames(K) == enhance.wpe_max_frames(K) >= 4096
    assert lib.vc_wpe_max_frames(32) == 6121 and lib.vc_wpe_max_frames(16) == 6644
    assert lib.vc_wpe_max_frames(0) == 0 and lib.vc_wpe_max_frames(33) == 0
    with pytest.raises(ValueError):
        enhance.wpe_max_frames(33)


def test_python_entry_points_refuse_bad_arguments_before_the_gpu():
    import audio_lib
    import enhance
    wav = np.zeros((2, 800), np.float32)
    for fn in (audio_lib.stft_complex_batch, enhance.dereverb_batch):
        name = fn.__name__
        for args, kw in (((np.zeros(800, np.float32), None), {}), ((wav, [800]), {}), ((wav, [800, 801]), {}),
                         ((wav, [800, -1]), {}), ((wav, None), dict(n_frames=[12, 3])), ((wav, None), dict(hop_length=0)),
                         ((wav, None), dict(n_fft=399)), ((wav, None), dict(n_fft=401)), ((wav, None), dict(win_length=2.5))):
            with pytest.raises(ValueError, match=name):
                fn(*args, **kw)
    with pytest.raises(ValueError, match='dereverb_batch: unknown dereverberation keyword'):
        enhance.dereverb_batch(wav, None, tap=3)
    with pytest.raises(ValueError, match='dereverb_batch: taps'):
        enhance.dereverb_batch(wav, None, taps=40)
    with pytest.raises(ValueError, match='at least hop_length'):
        enhance.dereverb_batch(np.zeros((1, 79), np.float32), None)
    long = np.zeros((1, 80 * 6200), np.float32)                       # 6201 frames: over the cap of 32 taps, under that of 16
    with pytest.raises(ValueError, match='vc_wpe_max_frames'):
        enhance.dereverb_batch(long, None, taps=32)
    re = np.zeros((2, 201, 30), np.float32)
    for args in ((re[0], re[0], None), (re, re[:, :, :29], None), (np.zeros((2, 1, 30), np.float32),) * 2 + (None,),
                 (re, re, [30]), (re, re, [30, 31]), (re, re, [3.0, 4.0])):
        with pytest.raises(ValueError, match='wpe_batch'):
            enhance.wpe_batch(*args)
    with pytest.raises(ValueError, match='wpe_batch: delay'):
        enhance.wpe_batch(re, re, None, delay=0)
    with pytest.raises(ValueError, match='vc_wpe_max_frames'):
        enhance.wpe_batch(np.zeros((1, 2, 6122), np.float32), np.zeros((1, 2, 6122), np.float32), None, taps=32)
    for args, kw in (((re, re, [30, 31]), {}), ((re[:, :200], re[:, :200], None), {}), ((re[:, :, :1], re[:, :, :1], None), {}),
                     ((re, re, None), dict(hop_length=401)), ((re, re, None), dict(n_fft=300))):
        with pytest.raises(ValueError, match='istft_complex_batch'):
            audio_lib.istft_complex_batch(*args, **kw)


def test_conversion_checks_dereverb_on_the_host():
    import conversion
    import inspect
    assert conversion._check_dereverb('t', None, CFG_D, 16000) is None and conversion._check_dereverb('t', False, CFG_D, 16000) is None
    c = conversion._check_dereverb('t', True, CFG_D, 16000)
    assert (c.taps, c.delay, c.iterations, c.context) == (16, 5, 3, 1)
    assert conversion._check_dereverb('t', dict(taps=8, iterations=1), CFG_D, 16000).taps == 8
    for bad, msg in ((3, 'must be None, True or a dict'), (dict(return_taps=True), 'return_taps is not offered'),
                     (dict(tap=1), 'unknown dereverberation keyword'), (dict(delay=99), 'delay')):
        with pytest.raises(ValueError, match=msg):
            conversion._check_dereverb('t', bad, CFG_D, 16000)
    with pytest.raises(ValueError, match='vc_wpe_max_frames'):
        conversion._check_dereverb('t', True, CFG_D, 80 * 7000)
    # every entry point that takes denoise= takes dereverb=, and None is its default
    n = 0
    for name, fn in inspect.getmembers(conversion, inspect.isfunction):
        par = inspect.signature(fn).parameters
        if name.startswith('convert_') and name.endswith('_batch') and 'denoise' in par:
            assert 'dereverb' in par and par['dereverb'].default is None, name
            n += 1
    assert n >= 8


def test_the_launches_validate_before_any_hip_call():
    """VC_ERR_INVALID with a message for every limit of vc_wpe_f32 and for NULL pointers of the two transforms: pure host
    code, no GPU."""
    import _vc
    lib = _vc.lib()
    p = C.c_void_p(4096)                                              # any non-NULL address: never dereferenced
    good = dict(taps=16, delay=5, iterations=3, context=1, floor_rel=1e-6, load_rel=1e-8)

    def call(batch=1, n_bins=201, max_frames=100, null=None, **kw):
        c = _vc.WpeCfg(**dict(good, **kw))
        a = dict(re=p, im=p, cfg=C.byref(c), out_re=p, out_im=p, status=p)
        if null:
            a[null] = None
        return lib.vc_wpe_f32(a['re'], a['im'], None, batch, n_bins, max_frames, a['cfg'], a['out_re'], a['out_im'], None,
                              a['status'], None)

    for kw in (dict(taps=0), dict(taps=33), dict(delay=0), dict(delay=65), dict(iterations=0), dict(iterations=17),
               dict(context=-1), dict(context=9), dict(floor_rel=0.0), dict(floor_rel=1.5), dict(floor_rel=float('nan')),
               dict(load_rel=-1e-9), dict(load_rel=1.5), dict(load_rel=float('nan')), dict(n_bins=1), dict(n_bins=2050),
               dict(batch=0), dict(batch=65536), dict(max_frames=0), dict(max_frames=6645), dict(max_frames=6122, taps=32),
               dict(null='re'), dict(null='im'), dict(null='cfg'), dict(null='out_re'), dict(null='out_im'), dict(null='status')):
        assert call(**kw) == 1 and b'vc_wpe_f32' in lib.vc_last_error(), kw
    assert lib.vc_stft_complex_f32(None, p, 10, p, None, 1, 5, p, p, p, None) == 1 and b'vc_stft_complex_f32' in lib.vc_last_error()
    assert lib.vc_istft_complex_f32(None, p, p, None, 1, 5, p, 320, p, 1 << 20, None) == 1
    assert b'vc_istft_complex_f32' in lib.vc_last_error()
    assert C.sizeof(_vc.WpeCfg) == 24


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('cid', ('edges-k4', 'ragged3', 'k1-d64'))
def test_restatement_scales_exactly_by_powers_of_two(cid):
    re, im, nf = dc.spectra(cid)
    cfg = dc.cfg_of(cid)
    base = ref.wpe_ref(re, im, nf, **cfg)
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all(), 'a frame at or beyond the count was read'
    for n in (-20, 3, 40):
        s = np.float32(2.0 ** n)
        got = ref.wpe_ref(re * s, im * s, nf, **cfg)
        assert np.array_equal(_bits(got[0]), _bits(base[0] * s)) and np.array_equal(_bits(got[1]), _bits(base[1] * s)), n
        assert np.array_equal(_bits(got[2]), _bits(base[2])) and np.array_equal(got[3], base[3]), n


def test_restatement_status_and_exact_passthrough():
    """edges-k4 holds F = 0 and F = D (status 2) next to F = D + 1 (status 0); the special bins hold the all-zero bin and the
    singular one.  Passthrough is bit for bit, the taps of a bin that was passed through are 0, frames at or beyond F are 0."""
    re, im, nf = dc.spectra('edges-k4')
    o_r, o_i, tp, st = ref.wpe_ref(re, im, nf, **dc.cfg_of('edges-k4'))
    assert st.tolist() == [[2] * 3, [2] * 3] + [[0] * 3] * 5
    for b, F in enumerate(nf):
        assert not o_r[b, :, F:].any() and not o_i[b, :, F:].any()
        if F <= 5:
            assert np.array_equal(_bits(o_r[b, :, :F]), _bits(re[b, :, :F])) and np.array_equal(_bits(o_i[b, :, :F]), _bits(im[b, :, :F]))
            assert not tp[b].any()
        else:
            assert tp[b].any() and not np.array_equal(_bits(o_r[b, :, :F]), _bits(re[b, :, :F]))
    re, im = dc.special_bins()
    kw = dict(taps=dc.SPECIAL_K, delay=dc.SPECIAL_D, iterations=3, context=1, floor_rel=1e-6)
    for load, want in ((1e-8, [1, 0, 0, 0, 0]), (0.0, [1, 0, 0, 1, 0])):
        o_r, o_i, tp, st = ref.wpe_ref(re, im, None, load_rel=load, **kw)
        assert st[0].tolist() == want, load
        for k in np.flatnonzero(st[0]):
            assert np.array_equal(_bits(o_r[0, k]), _bits(re[0, k])) and np.array_equal(_bits(o_i[0, k]), _bits(im[0, k]))
            assert not tp[0, k].any()
        # the constant bins are predicted exactly from frame D on (one tap of 1 would do; the least-squares solution spreads it)
        assert np.abs(o_r[0, 1, dc.SPECIAL_D + dc.SPECIAL_K:]).max() < 1e-6 and np.abs(o_r[0, 4, dc.SPECIAL_D + dc.SPECIAL_K:]).max() < 1e-6
        # bin 3: the impulse has nothing behind it to be predicted from; with the load it is solved and stays what it was
        if load > 0.0:
            assert np.array_equal(_bits(o_r[0, 3]), _bits(re[0, 3])) and not tp[0, 3].any() and st[0, 3] == 0


def test_restatement_is_a_function_of_its_own_utterance_and_bin():
    re, im, nf = dc.spectra('edges-k4')
    cfg = dc.cfg_of('edges-k4')
    whole = ref.wpe_ref(re, im, nf, **cfg)
    for b in (2, 6):
        alone = ref.wpe_ref(re[b:b + 1, 1:2], im[b:b + 1, 1:2], nf[b:b + 1], **cfg)
        for a, w in zip(alone, whole):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(w[b:b + 1, 1:2]).view(np.uint8))


def test_restatement_against_numpy_solve_on_its_own_normal_equations():
    """Guards the written-out factorisation: the taps against np.linalg.solve on the loaded R and q the restatement itself
    accumulated (the trace), to 1e-6 relative -- loose: cond(R) reaches 1e3 here and float32 taps carry 6e-8."""
    re, im, nf = dc.spectra('k16-ship')
    cfg = dict(dc.cfg_of('k16-ship'), iterations=1)
    trace = []
    _, _, tp, st = ref.wpe_ref(re[:1, :40], im[:1, :40], nf[:1], trace=trace, **cfg)
    assert not st.any()
    R, q = trace[0]
    g = np.linalg.solve(R, q[:, :, None])[:, :, 0]
    got = tp[0, :, :, 0].astype(np.float64) + 1j * tp[0, :, :, 1]
    assert np.abs(got - g).max() <= 1e-6 * np.abs(g).max()
    assert np.allclose(R, np.conj(np.swapaxes(R, 1, 2)))


# ------------------------------------------------------------------------------------------ the method, on the corpus
@pytest.mark.parametrize('t60', ref.T60S)
def test_restatement_on_the_room_corpus(t60):
    """T60 0.3 s and 0.6 s, DRR 6 dB, wpe_defaults (16 taps, delay 5), 3 iterations, context 1; SI-SDR against the early
    reference.  Measured here (float64 transforms; the float32 twin of the transforms in brackets):
        T60 0.3 s   12.469 -> 15.769 dB (+3.300)   [twin 15.769, |difference| < 1e-3 dB]
        T60 0.6 s    9.173 -> 11.809 dB (+2.635)   [twin 11.809, |difference| < 1e-3 dB]
    The issue's own script, on another corpus, gave +4.3 and +3.2 dB; its condition of 2 dB is kept as it stands (half of
    what this corpus gives would be 1.65 and 1.32 dB).  Every bin is solved (status 0); the loaded matrices' condition
    numbers reach 2.9e5 (median 1.1e4) and 7.9e4 (median 5.3e3): no float32 solve."""
    f = ref.corpus_figures(t60)
    gain, gap = f['si_out'] - f['si_in'], abs(f['si_twin'] - f['si_out'])
    print('MEASURED corpus T60 %.1f: SI-SDR %.3f -> %.3f dB (+%.3f), twin %.4f (|diff| %.2e dB), cond max %.3g median %.3g'
          % (t60, f['si_in'], f['si_out'], gain, f['si_twin'], gap, f['cond'].max(), np.median(f['cond'])))
    assert not f['status'].any() and not f['status_twin'].any()
    assert gain >= ref.MIN_GAIN_DB
    assert 2.0 * gap <= ref.E2E_FLOOR_DB, 'the twin is further off than the floor: the device margin is 2 x the gap, not the floor'
    assert 1e3 < f['cond'].max() < 1e7
