"""The vocoder kernels (csrc/vc_vocoder.hip) alone on the MI355X, one launch at a time, against the float64 reference of
tests/vocoder_kernels_ref.py on the configurations and inputs of tests/vocoder_kernels_cases.py.

Everything goes through the C ABI with plans of this file's own.  The caller-owned workspace (layout: include/vc_hip.h next
to vc_vocoder_workspace_bytes) holds what each part of a launch read and wrote: after num_iters launches frame buffer
num_iters & 1 holds the frames the last launch wrote, the other one the frames it read, and with momentum the state holds
the last launch's transform before the projection.  So the linear forward half, the projection with the linear inverse half,
and the overlap-add are each compared with float64 on the DEVICE'S OWN inputs, with the bounds of the float32 model stated in
the reference file; no comparison crosses a projection except the plain late launch, whose bound models it.

Every call: workspace filled with NaN, d_wav with a sentinel, wav_stride = L + 37, magnitudes and phases NaN in all rows at
or beyond an utterance's frame count, every buffer inside sentinel bands that are checked after the call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import vocoder_kernels_cases as vc
import vocoder_kernels_ref as ref

pytestmark = pytest.mark.gpu

BAND = 1024                                 # sentinel floats on each side of a guarded buffer
SENT = np.float32(-98765.4375)              # no kernel here computes this value
NAN = float('nan')
PLAIN, MOM = 'vc_griffin_lim_f32', 'vc_griffin_lim_momentum_f32'
SLACK = 37                                  # wav_stride - L


# ------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(autouse=True)
def _poisoned():
    poison_gpu_state()


class Guarded:
    """n float32 inside a larger device buffer whose bands hold the sentinel; .t is the inner view, filled with `fill`."""

    def __init__(self, n, fill=float(SENT), host=None):
        self.full = torch.full((n + 2 * BAND,), float(SENT), dtype=torch.float32, device='cuda')
        self.t = self.full[BAND:BAND + n]
        if host is not None:
            self.t.copy_(torch.from_numpy(np.array(host, dtype=np.float32).reshape(-1)))
        elif fill != float(SENT):
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.full[:BAND] == float(SENT)).all()) and bool((self.full[-BAND:] == float(SENT)).all()), \
            'sentinel band overwritten around ' + what

    def numpy(self):
        return self.t.cpu().numpy()


_PLANS = {}


def _plan_of(key, win, hop, n_fft, taps):
    import _vc
    if key not in _PLANS:
        h = C.c_void_p()
        _vc.check(_vc.lib().vc_vocoder_plan_create(win, hop, n_fft, _vc.ptr(taps), C.byref(h)))
        _PLANS[key] = (h, taps)                                   # the taps stay alive with the plan
    return _PLANS[key][0]


def _plan(cid):
    n_fft, win, hop, _ = vc.geometry(cid)
    return _plan_of(cid, win, hop, n_fft, vc.taps(cid))


@pytest.fixture(scope='module', autouse=True)
def _plans_destroyed_at_the_end():
    yield
    import _vc
    torch.cuda.synchronize()
    for h, _ in _PLANS.values():
        _vc.lib().vc_vocoder_plan_destroy(h)
    _PLANS.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _measured(what, got, want, bound):
    """One MEASURED line for the element with the worst error / bound; an element whose bound is 0 must be exact."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape
    assert np.isfinite(got).all(), what + ': the device value is not finite'
    err = np.abs(got - want)
    zero = bound <= 0.0
    assert not err[zero].any(), what + ': an element with bound 0 is not exact'
    if zero.all():
        print('MEASURED %s: error 0 bound 0 ratio 0.000 (all exact)' % what)
        return 0.0
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print('MEASURED %s: error %.3e bound %.3e ratio %.3f' % (what, err[i], bound[i], ratio[i]))
    assert ratio[i] <= 1.0, '%s: error %.3e > bound %.3e at %s' % (what, err[i], bound[i], i)
    return float(ratio[i])


class Result:
    pass


def _launch(entry, plan, n_fft, hop, amp, ph, n_frames, n, momentum, trace=False, ws_short=0, ws_shift=0, stride=None,
            max_frames=None, expect_ok=True):
    """One call of an entry point on guarded, poisoned buffers.  amp, ph [B, maxF, bins] float32 (host)."""
    import _vc
    lib = _vc.lib()
    B, maxF = amp.shape[:2]
    mf = maxF if max_frames is None else max_frames
    L = hop * (maxF - 1)
    stride = L + SLACK if stride is None else stride
    use_mom = entry == MOM and momentum > 0.0
    size = lib.vc_vocoder_workspace_bytes_momentum if use_mom else lib.vc_vocoder_workspace_bytes
    total = size(plan, B, mf, int(trace))
    lay = ref.ws_layout(n_fft, hop, B, maxF, int(trace), use_mom)
    if max_frames is None:
        assert total == lay[-1], (total, lay)
    else:
        total = lay[-1]
    d_amp, d_ph = Guarded(amp.size, host=amp), Guarded(ph.size, host=ph)
    d_wav = Guarded(B * max(stride, L + SLACK))
    d_ws = Guarded(total // 4 + 4, fill=NAN)
    d_tr = Guarded(n * B if n > 0 else B) if trace else None
    d_nf = None if n_frames is None else torch.tensor(list(n_frames), dtype=torch.int32, device='cuda')
    ws_ptr = C.c_void_p(d_ws.t.data_ptr() + ws_shift)
    args = [plan, _vc.ptr(d_amp.t), _vc.ptr(d_ph.t), _vc.ptr(d_nf), B, mf, n]
    if entry == MOM:
        args.append(float(momentum))
    args += [_vc.ptr(d_wav.t), stride, _vc.ptr(d_tr.t) if trace else None, ws_ptr, total - ws_short, _vc.current_stream()]
    rc = getattr(lib, entry)(*args)
    torch.cuda.synchronize()
    for g, what in ((d_amp, 'd_amp'), (d_ph, 'd_phase0'), (d_wav, 'd_wav'), (d_ws, 'the workspace')) + (((d_tr, 'd_trace'),) if trace else ()):
        g.check(what)
    assert _same_bits(d_amp.numpy(), amp.reshape(-1)) and _same_bits(d_ph.numpy(), ph.reshape(-1)), 'an input was written'
    r = Result()
    r.rc, r.err = rc, (lib.vc_last_error() or b'') if rc else b''
    r.B, r.maxF, r.L, r.stride, r.n = B, maxF, L, stride, n
    r.wav_raw = d_wav.numpy()
    r.ws_raw = d_ws.numpy()
    r.trace = d_tr.numpy().reshape(-1, B) if trace else None
    if not expect_ok:
        return r
    _vc.check(rc)
    ws = r.ws_raw
    fb, o_wav, wb, o_state, _ = lay
    assert np.isnan(ws[total // 4:]).all()
    r.wav = r.wav_raw[:B * stride].reshape(B, stride)
    assert (r.wav_raw[B * stride:] == SENT).all()
    r.fr = [ws[i * fb // 4:i * fb // 4 + B * maxF * n_fft].reshape(B, maxF, n_fft) for i in (0, 1)]
    r.wavs = [ws[(o_wav + i * wb) // 4:(o_wav + i * wb) // 4 + B * L].reshape(B, L) for i in (0, 1)] if trace else None
    r.state = None
    if use_mom:
        s = ref.state_slots(n_fft)
        st = ws[o_state // 4:o_state // 4 + B * maxF * s * 2].reshape(B, maxF, s, 2)
        r.state_raw = st
        r.state = st[..., 0].astype(np.float64) + 1j * st[..., 1].astype(np.float64)
    return r


@functools.lru_cache(maxsize=None)
def _run(cid, n, momentum):
    """The case's ragged batch through n launches; momentum None: the plain entry point."""
    n_fft, win, hop, frames = vc.geometry(cid)
    amp, ph = vc.inputs(cid)
    return _launch(PLAIN if momentum is None else MOM, _plan(cid), n_fft, hop, amp, ph, frames, n, momentum or 0.0)


def _untouched_beyond(r, frames, bufs):
    """Rows at or beyond an utterance's frame count keep the NaN fill in the given [B, maxF, ...] workspace views."""
    for a in bufs:
        for b, F in enumerate(frames):
            assert np.isnan(a[b, F:]).all(), 'a row beyond n_frames was written'


def _final(r):
    return r.fr[r.n & 1]


def _read_by_last(r):
    return r.fr[(r.n + 1) & 1]


# ------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize('cid', vc.ALL)
def test_workspace_sizes_equal_the_documented_layout(cid):
    import _vc
    lib = _vc.lib()
    n_fft, win, hop, frames = vc.geometry(cid)
    for B, maxF in ((len(frames), max(frames)), (1, frames[0]), (3, 129)):
        for trace in (0, 1):
            assert lib.vc_vocoder_workspace_bytes(_plan(cid), B, maxF, trace) == ref.ws_layout(n_fft, hop, B, maxF, trace, False)[-1]
            assert lib.vc_vocoder_workspace_bytes_momentum(_plan(cid), B, maxF, trace) == ref.ws_layout(n_fft, hop, B, maxF, trace, True)[-1]
    assert lib.vc_vocoder_workspace_bytes(_plan(cid), 0, 5, 0) == 0 and lib.vc_vocoder_workspace_bytes_momentum(_plan(cid), 2, 0, 0) == 0
    assert lib.vc_vocoder_num_samples(_plan(cid), frames[2]) == hop * (frames[2] - 1)


# ------------------------------------------------------------------------------------------ the initial launch
@pytest.mark.parametrize('cid', vc.ALL)
def test_init_launch_alone(cid):
    """num_iters == 1: the frames and the waveform are linear in amp * exp(i phase0).  Reaches: the initial kernel at every
    hop and window (its LDS does not depend on the hop), tiles with 1 .. 3 (generic) and 1 .. 15 valid frames, n_fft == 2
    (empty k loop), the > 64 KB launches, h_window."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    r = _run(cid, 1, None)
    assert np.isnan(r.fr[0]).all()                                   # one launch writes one frame buffer
    _untouched_beyond(r, frames, [r.fr[1]])
    for b, F in enumerate(frames):
        amp, ph = vc.single(cid, b)
        S = amp * np.exp(1j * ph)
        want = ref.frames_from_spectrum(S, w)
        fb = ref.inverse_bound(S, w)
        _measured('init frames %s utt %d' % (cid, b), r.fr[1][b, :F], want, fb)
        Lb = hop * (F - 1)
        wb = ref.trim(ref.ola_of_bound(fb, w, hop) + ref.ola_bound(want, w, hop), n_fft)
        _measured('init waveform %s utt %d' % (cid, b), r.wav[b, :Lb], ref.waveform(want, w, hop), wb)
        assert not r.wav[b, Lb:].any()


# ------------------------------------------------------------------------------------------ the forward half
def _prefix_is_bit_identical(cid, n, momentum):
    """The run of n - 1 launches is a prefix of the run of n: the frames both share are the same bits."""
    r, p = _run(cid, n, momentum), _run(cid, n - 1, momentum)
    assert _same_bits(_read_by_last(r), _final(p)), 'the run of n - 1 launches is not a prefix of the run of n'
    return r, p


@pytest.mark.parametrize('n', (2, 3, 5))
@pytest.mark.parametrize('cid', vc.ALL)
def test_forward_half_alone(cid, n):
    """The state after n launches, R_{n-1}, against the float64 analysis of the frames the last launch read.  Reaches:
    gather_tile / ola_at at every hop and nov (odd hop, nov 1, 2, 5, 58), win_length < n_fft on the 400-point kernel, the
    second arm of the window-sum rule (hop400), the asymmetric windows, MOM_FIRST (n = 2) and MOM_ON stores in slot order."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    r, _ = _prefix_is_bit_identical(cid, n, 0.99)
    _untouched_beyond(r, frames, [r.state_raw, r.fr[0], r.fr[1]])
    for b, F in enumerate(frames):
        fin = _read_by_last(r)[b, :F].astype(np.float64)
        R = ref.analysis(fin, w, hop)
        want = ref.slots_from_R400(R).reshape(F, -1) if n_fft == 400 else R
        bound = ref.forward_bound(fin, w, hop)[:, None]
        got = r.state[b, :F]
        _measured('forward re %s n=%d utt %d' % (cid, n, b), got.real, want.real, bound)
        _measured('forward im %s n=%d utt %d' % (cid, n, b), got.imag, want.imag, bound)


# ------------------------------------------------------------------------------------------ projection + inverse half
@pytest.mark.parametrize('momentum', (0.5, 0.99))
@pytest.mark.parametrize('n', (2, 3, 5))
@pytest.mark.parametrize('cid', vc.ALL)
def test_projection_and_inverse_alone(cid, n, momentum):
    """The frames the last launch wrote against float64 frames(amp * unit(C)), C = R_{n-1} - beta R_{n-2} formed in float64
    from the device's own float32 states (that of the run of n - 1 launches is R_{n-2}); n == 2 projects R_1 itself."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    r, p = _prefix_is_bit_identical(cid, n, momentum)
    beta = ref.beta_of(momentum)
    for b, F in enumerate(frames):
        amp, _ = vc.single(cid, b)
        Cx = r.state[b, :F] if n == 2 else r.state[b, :F] - beta * p.state[b, :F]
        if n_fft == 400:
            S = ref.slot_amp400(amp) * ref.unit(Cx.reshape(F, 13, 16))
            want = ref.frames_from_slots400(S, w)
            bound = ref.inverse_bound(ref.spectrum_from_slots400(S)[:, :201], w)
        else:
            S = ref.project(Cx, amp)
            want, bound = ref.frames_from_spectrum(S, w), ref.inverse_bound(S, w)
        _measured('projection+inverse %s n=%d m=%g utt %d' % (cid, n, momentum, b), _final(r)[b, :F], want, bound)


@pytest.mark.parametrize('cid', vc.ALL)
def test_plain_equals_first_momentum_launch_bitwise(cid):
    """Two launches: the plain flavour, the one production runs, writes the bits of the first momentum launch."""
    base = _run(cid, 2, None)
    for m in (0.5, 0.99):
        r = _run(cid, 2, m)
        assert _same_bits(r.fr[0], base.fr[0]) and _same_bits(r.fr[1], base.fr[1]) and _same_bits(r.wav, base.wav)
    one = _run(cid, 1, None)
    assert _same_bits(_read_by_last(base), _final(one))


@pytest.mark.parametrize('n', (3, 5))
@pytest.mark.parametrize('cid', vc.IN_CAP)
def test_plain_later_launch(cid, n):
    """The plain flavour's launch n against the float64 step of the frames it read, with the bound that models the
    projection's conditioning (tests/test_vocoder_kernels_cpu.py pins which cases stay under its cap)."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    r, _ = _prefix_is_bit_identical(cid, n, None)
    _untouched_beyond(r, frames, r.fr)
    for b, F in enumerate(frames):
        amp, _ = vc.single(cid, b)
        want, bound = ref.plain_step_bound(_read_by_last(r)[b, :F].astype(np.float64), amp, w, hop)
        _measured('plain launch %s n=%d utt %d' % (cid, n, b), _final(r)[b, :F], want, bound)


# ------------------------------------------------------------------------------------------ overlap-add
@pytest.mark.parametrize('cid', vc.ALL)
def test_overlap_add_alone(cid):
    """d_wav against the float64 overlap-add of the device's own final frames."""
    n_fft, win, hop, frames = vc.geometry(cid)
    w = vc.window(cid)
    for r in (_run(cid, 3, None), _run(cid, 2, 0.99)):
        for b, F in enumerate(frames):
            fr = _final(r)[b, :F].astype(np.float64)
            Lb = hop * (F - 1)
            assert not np.isnan(r.wav[b]).any()
            _measured('overlap-add %s utt %d' % (cid, b), r.wav[b, :Lb], ref.waveform(fr, w, hop), ref.trim(ref.ola_bound(fr, w, hop), n_fft))
            assert not r.wav[b, Lb:].any() and r.wav.shape[1] == hop * (max(frames) - 1) + SLACK
        assert not r.wav[len(frames) - 1].any() and not _final(r)[len(frames) - 1, :frames[-1]].any()


# ------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize('cid', vc.ALL)
def test_batch_equals_single_bitwise(cid):
    """An utterance in the ragged batch gives the bits of the same utterance run alone with d_n_frames == NULL."""
    n_fft, win, hop, frames = vc.geometry(cid)
    amp, ph = vc.inputs(cid)
    for m in (None, 0.99):
        r = _run(cid, 3, m)
        for b, F in enumerate(frames):
            s = _launch(PLAIN if m is None else MOM, _plan(cid), n_fft, hop, np.ascontiguousarray(amp[b:b + 1, :F]),
                        np.ascontiguousarray(ph[b:b + 1, :F]), None, 3, m or 0.0)
            Lb = hop * (F - 1)
            assert _same_bits(s.fr[0][0], r.fr[0][b, :F]) and _same_bits(s.fr[1][0], r.fr[1][b, :F])
            assert _same_bits(s.wav[0, :Lb], r.wav[b, :Lb]) and not s.wav[0, Lb:].any()
            if m is not None:
                assert _same_bits(s.state_raw[0], r.state_raw[b, :F])


@pytest.mark.parametrize('cid', ('ship', 'n16'))
def test_too_short_utterances_stay_in_bounds(cid):
    """The ABI clamps d_n_frames to min(max(n, 0), max_frames) and checks only max_frames against the reflect padding:
    utterances of 0, 1 and 2 frames, a negative count and one above max_frames sit next to valid ones.  From the code:
    gather_tile clamps its sample index to [0, L - 1] (to -1 for L == 0, where ola_at's sample n_fft / 2 - 1 is still
    inside frame 0) and ola_at clamps frame and offset, so every access stays inside the utterance's own rows."""
    n_fft, win, hop, frames = vc.geometry(cid)
    amp, ph = vc.inputs(cid)
    maxF = max(frames)
    assert hop * (2 - 1) <= n_fft // 2
    rows = [(1, frames[1]), (0, 0), (0, 1), (0, 2), (0, -3), (2, maxF + 5), (2, frames[2])]
    nf = [n for _, n in rows]
    a = np.stack([amp[u] for u, _ in rows])
    p = np.stack([ph[u] for u, _ in rows])
    for b, n in enumerate(nf):
        a[b, min(max(n, 0), maxF):] = NAN
        p[b, min(max(n, 0), maxF):] = NAN
    keep = [0, 5, 6]
    for entry, m in ((PLAIN, 0.0), (MOM, 0.99)):
        r = _launch(entry, _plan(cid), n_fft, hop, a, p, nf, 3, m)
        q = _launch(entry, _plan(cid), n_fft, hop, np.ascontiguousarray(a[keep]), np.ascontiguousarray(p[keep]),
                    [min(nf[b], maxF) for b in keep], 3, m)
        for i, b in enumerate(keep):
            assert _same_bits(r.fr[0][b], q.fr[0][i]) and _same_bits(r.fr[1][b], q.fr[1][i]) and _same_bits(r.wav[b], q.wav[i])
            if m:
                assert _same_bits(r.state_raw[b], q.state_raw[i])
            F = min(nf[b], maxF)
            assert np.isfinite(r.wav[b]).all() and np.isfinite(r.fr[1][b, :F]).all() and r.wav[b, :hop * (F - 1)].any()
        for b in (1, 2, 3, 4):
            F = min(max(nf[b], 0), maxF)
            Lb = max(hop * (F - 1), 0)
            assert np.isfinite(r.wav[b]).all() and not r.wav[b, Lb:].any()
            assert np.isfinite(r.fr[0][b, :F]).all() and np.isfinite(r.fr[1][b, :F]).all()
            assert np.isnan(r.fr[0][b, F:]).all() and np.isnan(r.fr[1][b, F:]).all()


# ------------------------------------------------------------------------------------------ trace
@pytest.mark.parametrize('n', (2, 3, 4))
@pytest.mark.parametrize('cid', ('ship', 'n16'))
def test_trace_rows(cid, n):
    """d_trace [num_iters, batch] in a ragged batch: the last two rows against the float64 sum of squared differences of the
    device's own waveforms (d_wav and the two scratch waveforms).  A float32 sum of L_b squares in any order:
    (L_b + 8) u relative; each difference is rounded once, which moves its square by 2 u."""
    n_fft, win, hop, frames = vc.geometry(cid)
    amp, ph = vc.inputs(cid)
    r = _launch(PLAIN, _plan(cid), n_fft, hop, amp, ph, frames, n, 0.0, trace=True)
    assert _same_bits(r.wav, _run(cid, n, None).wav)                    # tracing changes nothing
    assert r.trace.shape == (n, len(frames)) and not r.trace[0].any()
    seq = {n - 1: r.wav, n - 2: r.wavs[(n - 2) & 1]}
    if n >= 3:
        seq[n - 3] = r.wavs[(n - 3) & 1]
    for i in (n - 1, n - 2):
        if i < 1:
            continue
        for b, F in enumerate(frames):
            Lb = hop * (F - 1)
            d = seq[i][b, :Lb].astype(np.float64) - seq[i - 1][b, :Lb].astype(np.float64)
            want = float((d * d).sum())
            _measured('trace %s n=%d row %d utt %d' % (cid, n, i, b), r.trace[i, b], want, (Lb + 8 + 2) * ref.U * want)
    assert not r.trace[:, len(frames) - 1].any()


# ------------------------------------------------------------------------------------------ inverse pre-emphasis
def _preemph(plan, x, n_frames, max_frames, stride, coeff, target):
    import _vc
    g = Guarded(x.size, host=x)
    d_nf = torch.tensor(n_frames, dtype=torch.int32, device='cuda')
    _vc.check(_vc.lib().vc_inv_preemphasis_normalize(plan, _vc.ptr(g.t), _vc.ptr(d_nf), len(n_frames), max_frames, stride,
                                                     float(coeff), float(target), _vc.current_stream()))
    torch.cuda.synchronize()
    g.check('d_wav')
    return g.numpy().reshape(x.shape)


def _preemph_check(tag, x, got, Ls, coeff, target):
    c = float(np.float32(coeff))
    t = float(np.float32(target))
    for b, L in enumerate(Ls):
        assert _same_bits(got[b, L:], x[b, L:]), 'samples beyond the utterance changed'
        xin = x[b, :L].astype(np.float64)
        if L == 0:
            continue
        y, yb = ref.inv_preemphasis(xin, c), ref.inv_preemphasis_bound(xin, c)
        if c == 0.0:
            y, yb = xin, np.zeros(L)
        want, wb = ref.normalize(y, t), ref.normalize_bound(y, yb, t)
        if c == 0.0 and not t > 0:
            assert _same_bits(got[b, :L], x[b, :L])
        _measured('pre-emphasis %s L=%d' % (tag, L), got[b, :L], want, wb)
        if t > 0 and np.abs(xin).sum() > 0:
            mean = float(np.abs(got[b, :L].astype(np.float64)).mean())
            _measured('mean|y| %s L=%d' % (tag, L), mean, t, (ref.block_sum_terms(L) + 8 + 2) * ref.U * t)


def test_inverse_preemphasis_alone():
    """One block per utterance, each thread a chunk of ceil(L / 1024) samples: L < 1024 (most chunks empty), L == 0, the
    scan skipped (coeff == 0), a negative coefficient, the normalisation on its own, an all-zero row (tot == 0), and a row
    stride shorter than hop (F - 1)."""
    plan = _plan_of('preemph', 2, 1, 2, None)                          # hop 1: L = n_frames - 1
    Ls = [0, 1, 63, 1023, 1024, 1025, 4097, 500]
    maxF, stride = 4098, 4097 + SLACK
    rng = np.random.RandomState(11)
    x = (0.1 * rng.standard_normal((len(Ls), stride))).astype(np.float32)
    x[7, :500] = 0.0
    for coeff in (0.97, -0.97, 0.5, 0.0):
        for target in (0.0, 0.045):
            got = _preemph(plan, x, [L + 1 for L in Ls], maxF, stride, coeff, target)
            _preemph_check('c=%g t=%g' % (coeff, target), x, got, Ls, coeff, target)
            assert not got[7, :500].any()
    # a stride below hop (F - 1): the utterance ends at its row's end, and the next row is the next utterance's
    x = (0.1 * rng.standard_normal((3, 100))).astype(np.float32)
    got = _preemph(plan, x, [200, 50, 150], 200, 100, 0.97, 0.045)
    _preemph_check('stride 100', x, got, [100, 49, 100], 0.97, 0.045)


# ------------------------------------------------------------------------------------------ power -> amplitude
def _p2a(P, n_frames, norm, realse):
    import _vc
    B, maxF, nb = P.shape
    d_P, d_o = Guarded(P.size, host=P), Guarded(P.size)
    d_nf = torch.tensor(n_frames, dtype=torch.int32, device='cuda')
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(d_P.t), _vc.ptr(d_nf), B, maxF, nb, float(norm), float(realse), _vc.ptr(d_o.t),
                                        _vc.current_stream()))
    torch.cuda.synchronize()
    d_P.check('d_P')
    d_o.check('d_amp')
    return d_o.numpy().reshape(P.shape)


@pytest.mark.parametrize('nb', (2, 9, 201, 1025))
def test_power_to_amp_alone(nb):
    nf = [12, 7, 1, 5]
    rng = np.random.RandomState(nb)
    P = np.full((4, 12, nb), NAN, np.float32)
    for b, F in enumerate(nf):
        P[b, :F] = rng.uniform(-0.1, 0.9, (F, nb))
    P[0, 0, 0], P[2, 0, -1] = -0.05, 0.5                                 # something to clip; something above 0 in the one-frame utterance
    N = P.copy()
    N[3, :5] = -np.abs(N[3, :5])                                        # one utterance with nothing above 0
    N[3, 0, 0] = 0.0
    norm = float(np.float32(0.01))
    for realse in (1.0, 1.25, 0.8):
        rs = float(np.float32(realse))
        got, neg = _p2a(P, nf, 0.01, realse), _p2a(N, nf, 0.01, realse)
        for b, F in enumerate(nf):
            assert not got[b, F:].any() and not neg[b, F:].any()          # rows beyond n_frames: exactly 0
            want = ref.power_to_amp(P[b, :F].astype(np.float64), norm, rs)
            rel = ref.power_to_amp_rel_bound(P[b, :F].astype(np.float64), norm, rs)
            _measured('power_to_amp bins=%d realse=%g utt %d' % (nb, realse, b), got[b, :F], want, rel * want)
        # the reference's own 0 / 0: the utterance is NaN, the others do not notice
        assert _same_bits(neg[:3], got[:3])
        if realse == 1.0:
            _measured('power_to_amp bins=%d all clipped' % nb, neg[3, :5], np.full((5, nb), 1e-4), 8 * ref.U * 1e-4)
        else:
            assert np.isnan(ref.power_to_amp(N[3, :5].astype(np.float64), norm, rs)).all() and np.isnan(neg[3, :5]).all()


# ------------------------------------------------------------------------------------------ refusals
def test_plan_refusals():
    import _vc
    lib = _vc.lib()
    for win, hop, n_fft in ((401, 80, 401), (500, 80, 400), (4098, 1024, 4098), (400, 401, 400), (400, 0, 400), (400, -80, 400),
                            (4096, 4096, 4096)):
        h = C.c_void_p()
        rc = lib.vc_vocoder_plan_create(win, hop, n_fft, None, C.byref(h))
        assert rc != 0 and not h.value and b'vocoder' in lib.vc_last_error(), (win, hop, n_fft)
    assert ref.lds_bytes(4096, 4096) > 160 * 1024
    h = C.c_void_p()
    assert lib.vc_vocoder_plan_create(4096, 1024, 4096, None, C.byref(h)) == 0 and h.value      # the largest at that hop
    lib.vc_vocoder_plan_destroy(h)


@pytest.mark.parametrize('entry', (PLAIN, MOM))
@pytest.mark.parametrize('cid', ('ship', 'n16'))
def test_refusals_launch_nothing(cid, entry):
    """Every refusal of a run entry point: a non-zero code, vc_last_error names the entry point, and every output and the
    workspace keep their fill."""
    n_fft, win, hop, frames = vc.geometry(cid)
    amp, ph = vc.inputs(cid)
    F = frames[2]
    a, p = np.ascontiguousarray(amp[2:3]), np.ascontiguousarray(ph[2:3])
    L = hop * (F - 1)
    short = ref.min_frames(n_fft, hop) - 1
    bad = [('max_frames < 2', dict(max_frames=1), 3),
           ('too short for the reflect padding', dict(max_frames=short), 3),
           ('wav_stride < L', dict(stride=L - 1), 3),
           ('workspace one byte short', dict(ws_short=1), 3),
           ('num_iters == 0', dict(), 0)]
    if entry == MOM:
        bad.append(('momentum workspace off 16-byte alignment', dict(ws_shift=4), 3))
    for what, kw, n in bad:
        r = _launch(entry, _plan(cid), n_fft, hop, a, p, None, n, 0.5, expect_ok=False, **kw)
        assert r.rc != 0 and entry.encode() + b':' in r.err, (what, r.rc, r.err)
        assert (r.wav_raw == SENT).all() and np.isnan(r.ws_raw).all(), what
    good = _launch(entry, _plan(cid), n_fft, hop, a, p, None, 3, 0.5)
    assert good.rc == 0 and np.isfinite(good.wav).all()
