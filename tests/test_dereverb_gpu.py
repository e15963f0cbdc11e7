"""Dereverberation on the MI355X: vc_stft_complex_f32, vc_wpe_f32 and vc_istft_complex_f32 alone through the C ABI against
tests/dereverb_ref.py -- the solver bit for bit, the two transforms within the float32 bounds derived there --, identity
alone / in a batch / under graph replay, enhance.dereverb_batch end to end on the room corpus and dereverb= of the
conversion entry point a checkout can run.

Every kernel call as tests/test_denoise_gpu.py makes them: every buffer inside sentinel bands that are checked after the
call, outputs filled with NaN, spectrum frames at or beyond an utterance's count NaN, samples at or beyond its length NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import dereverb_cases as dc
import dereverb_ref as ref
import denoise_ref as dr
import diff_ref
import vocoder_kernels_cases as vc
from test_denoise_gpu import NAN, Guarded, _bits, _dev_i32, _measured, _power_batch, _power_call, _same_bits

pytestmark = pytest.mark.gpu

TRANSFORM_CASES = ('ship', 'n16', 'n512', 'skew16')          # 400-point tiles, two small generic ones, n_fft = 512: 257 bins
NAN_I32 = int(np.float32(NAN).view(np.int32))


@pytest.fixture(autouse=True)
def _poisoned():
    poison_gpu_state()


_PLANS = {}


def _plan(cid):
    import _vc
    if cid not in _PLANS:
        n_fft, win, hop, _ = vc.geometry(cid)
        h = C.c_void_p()
        _vc.check(_vc.lib().vc_vocoder_plan_create(win, hop, n_fft, _vc.ptr(vc.taps(cid)), C.byref(h)))
        _PLANS[cid] = h
    return _PLANS[cid]


@pytest.fixture(scope='module', autouse=True)
def _plans_destroyed_at_the_end():
    yield
    import _vc
    torch.cuda.synchronize()
    for h in _PLANS.values():
        _vc.lib().vc_vocoder_plan_destroy(h)
    _PLANS.clear()


# ------------------------------------------------------------------------------------------ the solver
def _wpe_call(re, im, nf, cfg, want_taps=True, null=None, **shape):
    """One vc_wpe_f32 call on guarded buffers: (rc, out_re, out_im [B, nb, maxF], taps [B, nb, K, 2] or None, status as int32
    bit patterns of the NaN-filled buffer)."""
    import _vc
    B, nb, maxF = re.shape
    K = cfg['taps']
    c = _vc.WpeCfg(K, cfg['delay'], cfg['iterations'], cfg['context'], cfg['floor_rel'], cfg['load_rel'])
    d_re, d_im = Guarded(re.size, host=re), Guarded(im.size, host=im)
    o_re, o_im = Guarded(re.size, fill=NAN), Guarded(re.size, fill=NAN)
    d_tp, d_st = Guarded(B * nb * K * 2, fill=NAN), Guarded(B * nb, fill=NAN)
    d_nf = _dev_i32(nf)
    p = dict(re=_vc.ptr(d_re.t), im=_vc.ptr(d_im.t), cfg=C.byref(c), out_re=_vc.ptr(o_re.t), out_im=_vc.ptr(o_im.t),
             status=_vc.ptr(d_st.t))
    if null:
        p[null] = None
    rc = _vc.lib().vc_wpe_f32(p['re'], p['im'], _vc.ptr(d_nf), shape.get('batch', B), shape.get('n_bins', nb),
                              shape.get('max_frames', maxF), p['cfg'], p['out_re'], p['out_im'],
                              _vc.ptr(d_tp.t) if want_taps else None, p['status'], _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_re, 'd_re'), (d_im, 'd_im'), (o_re, 'd_out_re'), (o_im, 'd_out_im'), (d_tp, 'd_taps'), (d_st, 'd_status')):
        g.check(what)
    assert _same_bits(d_re.numpy(), re.reshape(-1)) and _same_bits(d_im.numpy(), im.reshape(-1)), 'an input was written'
    if not want_taps:
        assert np.isnan(d_tp.numpy()).all(), 'taps were written through a NULL pointer'
    return (rc, o_re.numpy().reshape(re.shape), o_im.numpy().reshape(re.shape),
            d_tp.numpy().reshape(B, nb, K, 2) if want_taps else None, d_st.numpy().view(np.int32).reshape(B, nb))


def _assert_is_the_restatement(tag, got, want):
    rc, o_r, o_i, tp, st = got
    assert rc == 0, tag
    assert np.array_equal(st, want[3]), (tag, 'status', st.tolist(), want[3].tolist())
    for name, a, b in (('out_re', o_r, want[0]), ('out_im', o_i, want[1]), ('taps', tp, want[2])):
        if a is None:
            continue
        bad = np.flatnonzero(_bits(a).reshape(-1) != _bits(b).reshape(-1))
        assert bad.size == 0, '%s %s: %d of %d elements differ, first at %d: device %r restatement %r' % (
            tag, name, bad.size, a.size, bad[0], a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


@pytest.mark.parametrize('cid', dc.ALL)
def test_wpe_is_the_restatement_bit_for_bit(cid):
    """Outputs, taps and status of every case of tests/dereverb_cases.py against wpe_ref on the same float32 spectra: F = 0,
    D, D + 1, D + K - 1, D + K, 17, 33 and the frame cap; K = 1 .. 32; D = 1, 5, 64; 1 and 3 iterations; context 0 and 2;
    2, 3, 201 and 257 bins; ragged counts; max_frames no multiple of 16.  Frames at or beyond a count are NaN on the way in
    and 0 on the way out."""
    re, im, nf = dc.spectra(cid)
    cfg = dc.cfg_of(cid)
    want = ref.wpe_ref(re, im, nf, **cfg)
    got = _wpe_call(re, im, nf, cfg)
    _assert_is_the_restatement(cid, got, want)
    print('MEASURED wpe %s: %d bins solved, %d passed through, bit-identical' % (cid, int((got[4] == 0).sum()), int((got[4] != 0).sum())))


@pytest.mark.parametrize('load', (1e-8, 0.0))
def test_wpe_special_bins(load):
    """The all-zero bin (status 1), the constant bins (solved with and without the load: see tests/dereverb_cases.py), the
    singular bin (solved only because of the load; status 1 and exact passthrough without it), without the optional taps too."""
    re, im = dc.special_bins()
    cfg = dict(taps=dc.SPECIAL_K, delay=dc.SPECIAL_D, iterations=3, context=1, floor_rel=1e-6, load_rel=load)
    want = ref.wpe_ref(re, im, None, **cfg)
    assert want[3][0].tolist() == ([1, 0, 0, 0, 0] if load else [1, 0, 0, 1, 0])
    got = _wpe_call(re, im, None, cfg)
    _assert_is_the_restatement('special', got, want)
    for k in np.flatnonzero(got[4][0]):
        assert _same_bits(got[1][0, k], re[0, k]) and _same_bits(got[2][0, k], im[0, k]) and not got[3][0, k].any()
    _assert_is_the_restatement('special, no taps', _wpe_call(re, im, None, cfg, want_taps=False), want)


@pytest.mark.parametrize('cid', ('edges-k4', 'k16-ship'))
def test_wpe_scales_exactly_by_powers_of_two(cid):
    re, im, nf = dc.spectra(cid)
    cfg = dc.cfg_of(cid)
    base = _wpe_call(re, im, nf, cfg)
    for n in (-20, 40):
        s = np.float32(2.0 ** n)
        got = _wpe_call(re * s, im * s, nf, cfg)
        assert _same_bits(got[1], base[1] * s) and _same_bits(got[2], base[2] * s), n
        assert _same_bits(got[3], base[3]) and np.array_equal(got[4], base[4]), n


def test_wpe_alone_in_a_batch_and_under_graph_replay():
    """Every utterance of edges-k4 alone equals its rows in the batch; enhance._wpe_launch captured once and replayed with
    other spectra and counts copied into the static tensors equals eager calls on them."""
    import enhance
    from test_graph_replay_gpu import _capture, _free, _same
    re, im, nf = dc.spectra('edges-k4')
    cfg = dc.cfg_of('edges-k4')
    whole = _wpe_call(re, im, nf, cfg)
    for b in range(len(nf)):
        alone = _wpe_call(re[b:b + 1].copy(), im[b:b + 1].copy(), nf[b:b + 1], cfg)
        for a, w in zip(alone[1:], whole[1:]):
            assert _same_bits(a.astype(np.float32), w[b:b + 1].astype(np.float32)), b
    c = enhance.wpe_cfg('t', taps=4, delay=5, iterations=3, context=2)

    def inputs(k):
        r, i, _ = dc.spectra('edges-k4', seed=90 + k, poison=False)
        counts = np.roll(np.array(nf, np.int32), k)
        return [torch.from_numpy(r).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(counts).cuda()]

    static = inputs(0)
    g, outs = _capture(lambda: tuple(enhance._wpe_launch(static[0], static[1], static[2], c, True)))
    try:
        for k in (1, 2):
            new = inputs(k)
            for s, t in zip(static, new):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            want = enhance._wpe_launch(new[0], new[1], new[2], c, True)
            for name, a, b in zip(('re', 'im', 'status', 'taps'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert sorted(outs[2][:, 0].cpu().tolist()) == [0, 0, 0, 0, 0, 2, 2]
    finally:
        _free(g)


def test_wpe_refusals_launch_nothing():
    import _vc
    re, im, nf = dc.spectra('ragged3')
    cfg = dc.cfg_of('ragged3')
    for kw in (dict(cfg=dict(cfg, taps=33)), dict(cfg=dict(cfg, delay=0)), dict(cfg=dict(cfg, floor_rel=0.0)), dict(null='re'),
               dict(null='status'), dict(n_bins=1), dict(batch=0), dict(max_frames=ref.max_frames(2) + 1)):
        kw = dict(kw)
        rc, o_r, o_i, tp, st = _wpe_call(re, im, nf, kw.pop('cfg', cfg), **kw)
        assert rc == 1 and b'vc_wpe_f32' in _vc.lib().vc_last_error(), kw
        assert np.isnan(o_r).all() and np.isnan(o_i).all() and np.isnan(tp).all() and (st == NAN_I32).all(), kw


# ------------------------------------------------------------------------------------------ the transforms
def _stft_call(cid, wav, lens, nf, maxF):
    """One vc_stft_complex_f32 call on guarded buffers: (rc, re, im [B, nb, maxF], frame counts as int32 bit patterns)."""
    import _vc
    n_fft = vc.geometry(cid)[0]
    B, nb = wav.shape[0], 1 + n_fft // 2
    d_x, d_re, d_im, d_F = Guarded(wav.size, host=wav), Guarded(B * nb * maxF, fill=NAN), Guarded(B * nb * maxF, fill=NAN), Guarded(B, fill=NAN)
    d_len, d_nf = _dev_i32(lens), _dev_i32(nf)                          # held until the launch has run
    rc = _vc.lib().vc_stft_complex_f32(_plan(cid), _vc.ptr(d_x.t), wav.shape[1], _vc.ptr(d_len), _vc.ptr(d_nf), B, maxF,
                                       _vc.ptr(d_re.t), _vc.ptr(d_im.t), _vc.ptr(d_F.t), _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_x, 'd_wav'), (d_re, 'd_re'), (d_im, 'd_im'), (d_F, 'd_frames_out')):
        g.check(what)
    assert _same_bits(d_x.numpy(), wav.reshape(-1)), 'the waveform was written'
    return rc, d_re.numpy().reshape(B, nb, maxF), d_im.numpy().reshape(B, nb, maxF), d_F.numpy().view(np.int32)


def _ulps(a, b):
    """|a - b| in units of the float32 spacing at max(|a|, |b|, FLT_MIN)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(1.2e-38))).astype(np.float64)


@pytest.mark.parametrize('cid', TRANSFORM_CASES)
def test_stft_complex_ragged_batch_against_float64_and_the_power_launch(cid):
    """The ragged batch of the power launch's own test (a zero row, an exact multiple of hop, one more column than any
    utterance has frames -- no multiple of 16) and its frame counts.  Either component of every bin within
    (chain + 8) u sum |w x| of the float64 STFT (tests/dereverb_ref.py); frames at or beyond F_b are 0; d_frames_out equals
    vc_stft_power_f32's on the same input; re^2 + im^2 within ref.POWER_ULPS float32 ulps of that launch's power."""
    n_fft, win, hop, _ = vc.geometry(cid)
    w = vc.window(cid)
    wav, lens, _, _ = _power_batch(cid)
    full = [1 + n // hop for n in lens]
    maxF = max(full) + 1
    for tag, nf in (('null', None), ('cut', [full[0] - 1, full[1], 5]), ('above-negative', [full[0] + 3, -2, 0])):
        rc, re, im, Fout = _stft_call(cid, wav, lens, nf, maxF)
        rc_p, P, Fp = _power_call(cid, wav, lens, nf, maxF)
        assert rc == 0 and rc_p == 0 and Fout.tolist() == Fp.tolist(), (tag, Fout.tolist(), Fp.tolist())
        worst = 0.0
        for b, n in enumerate(lens):
            F = dr.frames_of(n, None if nf is None else nf[b], maxF, n_fft, hop)
            assert int(Fout[b]) == F, (tag, b)
            assert not re[b, :, F:].any() and not im[b, :, F:].any() and not np.isnan(re[b]).any() and not np.isnan(im[b]).any()
            if F:
                x = wav[b, :n].astype(np.float64)
                Z = ref.stft(x, w, hop, F)
                e = np.broadcast_to(ref.stft_bound(x, w, hop, F)[None, :], Z.shape)
                _measured('stft %s %s utt %d re' % (cid, tag, b), re[b, :, :F], Z.real, e)
                _measured('stft %s %s utt %d im' % (cid, tag, b), im[b, :, :F], Z.imag, e)
                p2 = (re[b, :, :F] * re[b, :, :F] + im[b, :, :F] * im[b, :, :F]).astype(np.float32)
                worst = max(worst, float(_ulps(p2.T, P[b, :F]).max()))
        print('MEASURED stft %s %s: re^2 + im^2 against the power launch, worst %.2f ulps' % (cid, tag, worst))
        assert worst <= ref.POWER_ULPS, (cid, tag, worst)


def _istft_call(cid, re, im, nf, out_stride=None):
    """One vc_istft_complex_f32 call on guarded buffers: (rc, y [B, out_stride])."""
    import _vc
    lib = _vc.lib()
    n_fft, _, hop, _ = vc.geometry(cid)
    B, nb, maxF = re.shape
    stride = hop * (maxF - 1) + 3 if out_stride is None else out_stride
    nws = lib.vc_stft_filter_workspace_bytes(_plan(cid), B, maxF)
    d_re, d_im, d_y, d_ws = Guarded(re.size, host=re), Guarded(im.size, host=im), Guarded(B * stride, fill=NAN), Guarded(nws // 4, fill=NAN)
    d_nf = _dev_i32(nf)                                                 # held until the launch has run
    rc = lib.vc_istft_complex_f32(_plan(cid), _vc.ptr(d_re.t), _vc.ptr(d_im.t), _vc.ptr(d_nf), B, maxF, _vc.ptr(d_y.t), stride,
                                  _vc.ptr(d_ws.t), nws, _vc.current_stream())
    torch.cuda.synchronize()
    for g, what in ((d_re, 'd_re'), (d_im, 'd_im'), (d_y, 'd_out'), (d_ws, 'workspace')):
        g.check(what)
    assert _same_bits(d_re.numpy(), re.reshape(-1)) and _same_bits(d_im.numpy(), im.reshape(-1)), 'an input was written'
    return rc, d_y.numpy().reshape(B, stride)


@pytest.mark.parametrize('cid', TRANSFORM_CASES)
def test_istft_complex_ragged_batch_against_float64(cid):
    """Spectra of noise (so: nothing a forward transform would produce, imaginary parts at bin 0 and bin N / 2 included --
    they must be ignored) over the case's ragged frame counts, a count of 0, one under the reflect padding and a NULL count;
    frames at or beyond a count NaN.  hop (F - 1) samples within the inverse half's bound of the float64 ISTFT, zeros up to
    out_stride, every element written."""
    n_fft, _, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    nb, maxF = 1 + n_fft // 2, max(frames) + 1
    short = max(1, (n_fft // 2) // hop)                                  # hop (short - 1) <= n_fft / 2
    nf = list(frames[:3]) + [0, short]
    rng = np.random.RandomState(41)
    re = rng.standard_normal((len(nf), nb, maxF)).astype(np.float32)
    im = rng.standard_normal((len(nf), nb, maxF)).astype(np.float32)
    for b, F in enumerate(nf):
        re[b, :, F:], im[b, :, F:] = NAN, NAN
    rc, y = _istft_call(cid, re, im, nf)
    assert rc == 0 and not np.isnan(y).any()
    for b, F in enumerate(nf):
        F = 0 if hop * (F - 1) <= n_fft // 2 else F
        n = hop * max(F - 1, 0)
        assert not y[b, n:].any(), (cid, b)
        if F:
            want, bound = ref.istft_bound(re[b, :, :F].astype(np.float64) + 1j * im[b, :, :F].astype(np.float64), w, hop)
            _measured('istft %s utt %d (F %d)' % (cid, b, F), y[b, :n], want, bound)
    full = np.nan_to_num(re[:1]), np.nan_to_num(im[:1])
    rc, y0 = _istft_call(cid, full[0], full[1], None, out_stride=hop * (maxF - 1))
    want, bound = ref.istft_bound(full[0][0].astype(np.float64) + 1j * full[1][0].astype(np.float64), w, hop)
    assert rc == 0
    _measured('istft %s NULL counts' % cid, y0[0], want, bound)


@pytest.mark.parametrize('cid', ('ship', 'n512'))
def test_round_trip_against_the_unit_gain_filter(cid):
    """istft(stft(x)) against stft_filter_batch(gain = 1) on the power test's ragged batch.  Recorded on the MI355X: on the
    generic path (n512) the two are bit-identical, and that is asserted; on the 400-point path (ship) they are not (largest
    difference 4.5e-8, one rounding, at a peak of 0.4).  Why: the filter kernel keeps its own in-line text of the two halves
    -- moved onto shared functions it compiles to other contractions and its output changes in the last bit, which an older
    launch must not -- and the inverse half here is a function, so the compiler fuses other products into other sums.
    Asserted in both cases: the same frame counts and zeros, and both within the filter's own float64 bound
    (tests/diff_ref.py filter_bound with G = 1) of the float64 filter."""
    import audio_lib
    n_fft, win, hop, _ = vc.geometry(cid)
    w = vc.window(cid)
    wav, lens, _, _ = _power_batch(cid)
    clean = np.nan_to_num(wav)
    kw = dict(win_length=win, hop_length=hop, n_fft=n_fft)
    re, im, d_F = audio_lib.stft_complex_batch(clean, lens, **kw)
    y = audio_lib.istft_complex_batch(re, im, d_F, **kw).cpu().numpy()
    maxF = re.shape[2]
    yf = audio_lib.stft_filter_batch(clean, lens, torch.ones((3, maxF, 1 + n_fft // 2), device='cuda'), d_F, **kw).cpu().numpy()
    assert y.shape == yf.shape
    print('MEASURED round trip %s: bit-identical to the unit-gain filter: %s (largest difference %.3e)' % (
        cid, _same_bits(y, yf), np.abs(y.astype(np.float64) - yf).max()))
    if n_fft != 400:
        assert _same_bits(y, yf), 'the generic path shares both sums with the filter kernel'
    for b, F in enumerate(d_F.cpu().tolist()):
        n = hop * max(F - 1, 0)
        assert not y[b, n:].any() and not yf[b, n:].any()
        if F:
            want, bound = diff_ref.filter_bound(wav[b, :lens[b]].astype(np.float64), np.ones((F, 1 + n_fft // 2)), w, hop, n_use=F)
            _measured('round trip %s utt %d' % (cid, b), y[b, :n], want, bound)
            _measured('unit-gain filter %s utt %d' % (cid, b), yf[b, :n], want, bound)


def test_transform_refusals_launch_nothing():
    import _vc
    lib = _vc.lib()
    d = Guarded(4096, fill=NAN)
    p = _vc.ptr(d.t)
    st = _vc.current_stream()
    for args in ((None, p, 100, p, None, 1, 2, p, p, p, st), (_plan('ship'), None, 100, p, None, 1, 2, p, p, p, st),
                 (_plan('ship'), p, 100, p, None, 0, 2, p, p, p, st), (_plan('ship'), p, 100, p, None, 1, 0, p, p, p, st),
                 (_plan('ship'), p, 0, p, None, 1, 2, p, p, p, st), (_plan('ship'), p, 100, p, None, 1, 2, p, None, p, st)):
        assert lib.vc_stft_complex_f32(*args) == 1 and b'vc_stft_complex_f32' in lib.vc_last_error()
    nws = lib.vc_stft_filter_workspace_bytes(_plan('ship'), 1, 4)
    for args, code in (((None, p, p, None, 1, 4, p, 240, p, nws, st), 1), ((_plan('ship'), p, None, None, 1, 4, p, 240, p, nws, st), 1),
                       ((_plan('ship'), p, p, None, 1, 4, p, 239, p, nws, st), 1), ((_plan('ship'), p, p, None, 1, 0, p, 240, p, nws, st), 1),
                       ((_plan('ship'), p, p, None, 1, 4, p, 240, p, nws - 1, st), 3)):
        assert lib.vc_istft_complex_f32(*args) == code and b'vc_istft_complex_f32' in lib.vc_last_error()
    torch.cuda.synchronize()
    d.check('the buffer')
    assert np.isnan(d.numpy()).all()


# ------------------------------------------------------------------------------------------ Python, end to end
def test_python_entry_points_are_the_launches_and_wait_for_nothing():
    """stft_complex_batch, wpe_batch, istft_complex_batch and dereverb_batch under set_sync_debug_mode('error'): each equals
    the C call on guarded buffers, and dereverb_batch equals the three in a row."""
    import audio_lib
    import enhance
    wav, lens, _, _ = _power_batch('ship')
    clean = torch.from_numpy(np.nan_to_num(wav)).cuda()
    d_len = torch.tensor(lens, dtype=torch.int32, device='cuda')
    kw = dict(taps=4, delay=5, iterations=2, context=1)
    enhance.dereverb_batch(clean, d_len, **kw)                          # warm-up: the plan, the library, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        re, im, d_F = audio_lib.stft_complex_batch(clean, d_len)
        r = enhance.wpe_batch(re, im, d_F, return_taps=True, **kw)
        y = audio_lib.istft_complex_batch(r.re, r.im, d_F)
        whole = enhance.dereverb_batch(clean, d_len, return_taps=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    maxF = 1 + wav.shape[1] // 80
    rc, c_re, c_im, c_F = _stft_call('ship', wav, lens, None, maxF)
    assert tuple(re.shape) == (3, 201, maxF) and _same_bits(re.cpu().numpy(), c_re) and _same_bits(im.cpu().numpy(), c_im)
    assert d_F.cpu().tolist() == c_F.tolist() and c_F[2] == 0
    cfg = dict(taps=4, delay=5, iterations=2, context=1, floor_rel=1e-6, load_rel=1e-8)
    got = _wpe_call(c_re, c_im, c_F.tolist(), cfg)
    for a, b in ((r.re, got[1]), (r.im, got[2]), (r.taps, got[3])):
        assert _same_bits(a.cpu().numpy(), b)
    assert np.array_equal(r.status.cpu().numpy(), got[4]) and not got[4][:2].any() and (got[4][2] == 2).all()
    rc, c_y = _istft_call('ship', got[1], got[2], c_F.tolist(), out_stride=80 * (maxF - 1))
    assert _same_bits(y.cpu().numpy(), c_y)
    for a, b in ((whole.y, y), (whole.n_frames, d_F), (whole.status, r.status), (whole.taps, r.taps)):
        assert torch.equal(a, b)
    assert enhance.dereverb_batch(clean, d_len, **kw).taps is None


def test_dereverb_batch_on_the_room_corpus():
    """Both rooms (T60 0.3 s and 0.6 s, DRR 6 dB) in one batch through enhance.dereverb_batch at its defaults -- wpe_defaults
    (16, 5), 3 iterations, context 1 -- scored on the device by evaluation.si_sdr_batch against the early reference.
    The restatement (tests/test_dereverb_cpu.py, measured there): 12.469 -> 15.769 dB and 9.173 -> 11.809 dB; its float32
    twin of the transforms differs from it by 1.0e-6 and 2.9e-7 dB, so the margin between device and restatement is the floor,
    0.05 dB.  The improvement must be at least 2 dB in both rooms, and every bin solved."""
    import enhance
    import evaluation
    figs = [ref.corpus_figures(t) for t in ref.T60S]
    rev = torch.from_numpy(np.stack([f['rev'] for f in figs])).cuda()
    early = torch.from_numpy(np.stack([f['early'] for f in figs])).cuda()
    n = figs[0]['n']
    assert n == rev.shape[1]
    d_len = torch.full((2,), n, dtype=torch.int32, device='cuda')
    enhance.dereverb_batch(rev, d_len)                                  # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = enhance.dereverb_batch(rev, d_len)
        before = evaluation.si_sdr_batch(early, rev, d_len)
        after = evaluation.si_sdr_batch(early, r.y, d_len)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tuple(r.y.shape) == (2, n) and r.n_frames.cpu().tolist() == [1 + n // 80] * 2
    assert not bool(r.status.any()), 'a bin of the corpus was not solved'
    b, a = before.si_sdr.cpu().numpy().astype(np.float64), after.si_sdr.cpu().numpy().astype(np.float64)
    for k, f in enumerate(figs):
        margin = max(2.0 * abs(f['si_twin'] - f['si_out']), ref.E2E_FLOOR_DB)
        print('MEASURED dereverb_batch T60 %.1f: SI-SDR %.4f -> %.4f dB on the device, %.4f -> %.4f the restatement (margin %.3f)'
              % (ref.T60S[k], b[k], a[k], f['si_in'], f['si_out'], margin))
        assert abs(a[k] - f['si_out']) <= margin and abs(b[k] - f['si_in']) <= ref.E2E_FLOOR_DB
        assert a[k] - b[k] >= ref.MIN_GAIN_DB


def test_convert_gmm_diff_batch_with_dereverb():
    """convert_gmm_diff_batch(dereverb=True) equals, bit for bit, convert_gmm_diff_batch applied to dereverb_batch's output
    cut the same way (lengths to whole hops); with dereverb=None (and False) its output is today's; dereverb and denoise
    together are dereverb first."""
    import conversion
    import enhance
    import mapping
    import mapping_cases as mc
    import mapping_ref as mr
    m = mr.random_model(4, 48, seed=3, spread=0.25)
    model = mapping.JDGMM(*(torch.from_numpy(m[k]).cuda() for k in mr.FIELDS))
    f = ref.corpus_figures(0.3)
    lens = [16000 + 37, 12000]
    wav = torch.from_numpy(np.stack([f['rev'][:lens[0]], np.concatenate([f['rev'][4000:16000], np.zeros(4037, np.float32)])])).cuda()
    plain = conversion.convert_gmm_diff_batch(model, wav, lens, mc.CFG)
    for off in (None, False):
        again = conversion.convert_gmm_diff_batch(model, wav, lens, mc.CFG, dereverb=off)
        assert torch.equal(again.y_wav_pred, plain.y_wav_pred) and again.n_samples == plain.n_samples
    got = conversion.convert_gmm_diff_batch(model, wav, lens, mc.CFG, dereverb=True)
    cut = [80 * (n // 80) for n in lens]
    d = enhance.dereverb_batch(wav, cut)
    want = conversion.convert_gmm_diff_batch(model, d.y, cut, mc.CFG)
    assert got.n_samples == want.n_samples == cut and got.n_frames == want.n_frames
    for name in ('y_wav_pred', 'mel_true', 'cep_src', 'cep_pred', 'gain'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert not torch.equal(got.y_wav_pred[:, :cut[1]], plain.y_wav_pred[:, :cut[1]]) and bool(torch.isfinite(got.y_wav_pred).all())
    kw = dict(taps=8, iterations=1)
    both = conversion.convert_gmm_diff_batch(model, wav, lens, mc.CFG, dereverb=kw, denoise=True)
    d8 = enhance.dereverb_batch(wav, cut, **kw)
    want = conversion.convert_gmm_diff_batch(model, d8.y, cut, mc.CFG, denoise=True)
    assert torch.equal(both.y_wav_pred, want.y_wav_pred)
