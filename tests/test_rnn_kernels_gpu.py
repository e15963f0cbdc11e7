"""Every entry point of csrc/vc_rnn.hip alone (vc_gru_bidir and its five kernels, vc_lstm_bidir, vc_softmax_argmax,
vc_softmax_argmax_dual, vc_convert), called through _vc.lib() and compared with the float64 definitions of
tests/rnn_ref.py at the sizes where the host code or a kernel takes another path.  Inputs, shape tables and bounds come
from tests/test_rnn_kernels_cpu.py, which proves them usable without a device.  Output buffers are NaN-filled and end in
a NaN row that must survive; the GRU workspace is exactly vc_gru_workspace_bytes long and followed by a canary; every
test starts from and leaves gru_mfma = -1.  Lines starting with 'MEASURED' carry the device's worst error next to its
bound (profiles/rnn_kernels/README.md records them).

Bounds: rnn_bound() of the CPU file -- max(k x |restatement - float64| on the same input, 1e-6), k = 8 for float32
arithmetic and 4 for the kernels whose bf16 roundings the restatement repeats, plus 2^-8 |expected| when the output is
bf16; never above the suite's flat 3e-2 (bf16) / 5e-5 (float32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnn_ref as R
from conftest import poison_gpu_state
from test_rnn_kernels_cpu import (BOTH, CONVERT_N, GRU_GROUPS, LSTM_GROUPS, SOFTMAX_M, SOFTMAX_N, SOFTMAX_TIES, VC_BF16, VC_F32,
                                  case_of, convert_specials, convert_subnormals, gru_bf16_state, gru_kernel, reversed_case,
                                  rnn_bound, rnn_case, softmax_logits, unreverse)

pytestmark = pytest.mark.gpu

VC_ERR_INVALID, VC_ERR_WORKSPACE = 1, 3
TORCH_DT = {VC_F32: torch.float32, VC_BF16: torch.bfloat16}
NAME = {VC_F32: 'f32', VC_BF16: 'bf16'}
CANARY = 0xA5


def _lib():
    import _vc
    return _vc.lib()


def _st():
    import _vc
    return _vc.current_stream()


def _check(rc):
    import _vc
    _vc.check(rc)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a, dtype=VC_F32):
    """numpy float32 -> device tensor of the library dtype (bf16: the array must already be on the bf16 grid)."""
    t = torch.from_numpy(np.array(a, dtype=np.float32))
    if dtype == VC_BF16:
        assert np.array_equal(R.to_bf16(a), a)
        t = t.bfloat16()
    return t.cuda()


def nans(rows, cols, dtype):
    return torch.full((rows, cols), float('nan'), dtype=TORCH_DT[dtype], device='cuda')


def raw(t):
    """The tensor's bits on the host."""
    torch.cuda.synchronize()
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().copy()


def val(t):
    torch.cuda.synchronize()
    return t.detach().cpu().to(torch.float64).numpy()


@pytest.fixture(autouse=True)
def _default_options():
    import _vc
    assert _vc.get_option('gru_mfma') == -1
    yield
    _vc.set_option('gru_mfma', -1)
    assert _vc.get_option('gru_mfma') == -1


# ------------------------------------------------------------------------------------------ recurrences

def _run(cell, xp, wf, wb, T, w_dtype, out_dtype, ws_bytes='exact', expect=0):
    """One launch: returns the output tensor [rows, 2H] (tail row, workspace canary checked)."""
    lib = _lib()
    H, rows = wf.shape[0], xp.shape[0]
    n_seq = rows // T
    xd, wfd, wbd = dev(xp), dev(wf, w_dtype), dev(wb, w_dtype)
    out = nans(rows + 1, 2 * H, out_dtype)
    if cell == 'gru':
        need = int(lib.vc_gru_workspace_bytes(H, w_dtype))
        assert need == 2 * 3 * H * H * (4 if w_dtype == VC_F32 else 2)
        ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device='cuda')
        give = need if ws_bytes == 'exact' else ws_bytes
        rc = lib.vc_gru_bidir(p(xd), p(wfd), p(wbd), w_dtype, n_seq, T, H, p(out), out_dtype,
                              None if give is None else p(ws), 0 if give is None else give, _st())
    else:
        ws, need = None, 0
        rc = lib.vc_lstm_bidir(p(xd), p(wfd), p(wbd), w_dtype, n_seq, T, H, p(out), out_dtype, _st())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib().vc_last_error())
    if ws is not None:
        assert bool((ws[need:] == CANARY).all()), 'wrote past vc_gru_workspace_bytes'
        if expect:
            assert bool((ws == CANARY).all()), 'a refused call wrote the workspace'
    assert bool(torch.isnan(out[rows:].float()).all()), 'wrote past the last row'
    return out[:rows]


def _recurrence_group(cell, name, gm, rows):
    """All cases of one group, every (w_dtype given, out_dtype) pair; then the same launches again after
    poison_gpu_state(), bit for bit."""
    import _vc
    _vc.set_option('gru_mfma', gm)
    poison_gpu_state()
    first = {}
    failures = []
    for row in rows:
        c = case_of(cell, row)
        H, T, n_seq, w = c['H'], c['T'], c['n_seq'], c['w_dtype']
        st = gru_bf16_state(gru_kernel(H, w, n_seq, gm), w) if cell == 'gru' else False
        x2, wf2, wb2 = reversed_case(c['xproj'], c['wf'], c['wb'], T)
        for od in BOTH:
            out = _run(cell, c['xproj'], c['wf'], c['wb'], T, w, od)
            got, bits = val(out), raw(out)
            first[(row, od)] = bits
            bound, cap = rnn_bound(c, st, od)
            assert float(bound.max()) <= cap
            err = np.abs(got - c['want'])
            print('MEASURED %s %s H=%d T=%d n_seq=%d w=%s out=%s %s err=%.2e bound=%.2e'
                  % (cell, name.split('-')[0], H, T, n_seq, NAME[w], NAME[od], row[4], float(np.nanmax(err)) if err.size else 0.0,
                     float(bound.max())))
            ok = np.isfinite(got).all() and float(np.abs(got).max()) <= 1.0 and bool((err <= bound).all())
            if not ok:
                failures.append((row, NAME[od], 'finite=%s max|h|=%g err=%g bound=%g' % (np.isfinite(got).all(), np.nanmax(np.abs(got)),
                                                                                         np.nanmax(err), bound.max())))
            # the backward direction is the forward direction of the reversed input with the weights swapped
            back = unreverse(raw(_run(cell, x2, wf2, wb2, T, w, od)), T)
            if not np.array_equal(back, bits):
                failures.append((row, NAME[od], 'direction reversal: %d elements differ' % int((back != bits).sum())))
    poison_gpu_state()
    for row in rows:
        c = case_of(cell, row)
        for od in BOTH:
            again = raw(_run(cell, c['xproj'], c['wf'], c['wb'], c['T'], c['w_dtype'], od))
            if not np.array_equal(again, first[(row, od)]):
                failures.append((row, NAME[od], 'second call differs in %d elements' % int((again != first[(row, od)]).sum())))
    assert not failures, failures


@pytest.mark.parametrize('name', sorted(GRU_GROUPS))
def test_gru_bidir_against_float64(name):
    """vc_gru_bidir, one group of tests/test_rnn_kernels_cpu.py:GRU_GROUPS per test: the generic kernel at H = 1 .. 1024
    (KS = 64 at 1; KS1 2 -> 1 at 64 / 65; block 256 -> 512 at 128 / 129; weights in LDS or not at 112 / 113 (float32) and
    159 / 160 (bf16); more than one column per thread group from 257, which the kernel did not compute before it looped:
    gate columns 512 .. 2H - 1 were never written), the wave kernel with partly filled four-wave workgroups, the
    register-resident kernels, the MFMA kernel with a clamped last 16-sequence slot.  T = 1 and 2 beside an ordinary T;
    float32 and bf16 outputs for each weight dtype; random and saturated inputs (gates at +-40 and +-100, where __expf
    underflows and overflows): finite, |h| <= 1, within the bound; backward = forward of the reversed input, bit for bit;
    a second call after poison_gpu_state() bit for bit."""
    gm, rows = GRU_GROUPS[name]
    _recurrence_group('gru', name, gm, rows)


@pytest.mark.parametrize('name', sorted(LSTM_GROUPS))
def test_lstm_bidir_against_float64(name):
    """vc_lstm_bidir at H = 1, 40, both sides of the weights-in-LDS threshold (97 / 98 float32, 137 / 138 bf16) and the
    largest admitted size 512; T = 1, 2 and ordinary; n_seq 1 and 3; same checks as the GRU groups."""
    _recurrence_group('lstm', name, -1, LSTM_GROUPS[name])


@pytest.mark.parametrize('H', [128, 256])
def test_gru_default_dispatch_is_the_forced_form_bit_for_bit(H):
    """gru_mfma = -1: 31 sequences take the VALU form, 32 the MFMA form."""
    import _vc
    for n_seq, forced in ((31, 0), (32, 1)):
        c = rnn_case('gru', H, 3, n_seq, VC_BF16)
        res = {}
        for gm in (-1, 0, 1):
            _vc.set_option('gru_mfma', gm)
            res[gm] = raw(_run('gru', c['xproj'], c['wf'], c['wb'], 3, VC_BF16, VC_F32))
        assert np.array_equal(res[-1], res[forced]), (n_seq, 'default is not the form the threshold names')
        assert not np.array_equal(res[0], res[1]), 'the two forms cannot be told apart on this input'
        bound, _ = rnn_bound(c, True, VC_F32)
        for gm in (0, 1):
            got = res[gm].view(np.float32).astype(np.float64)
            assert bool((np.abs(got - c['want']) <= bound).all()), (n_seq, gm)


@pytest.mark.parametrize('H,w_dtype,gm', [(128, VC_BF16, 0), (256, VC_BF16, 0), (128, VC_BF16, 1), (256, VC_BF16, 1), (128, VC_F32, -1)])
def test_gru_short_or_missing_workspace_is_refused(H, w_dtype, gm):
    import _vc
    _vc.set_option('gru_mfma', gm)
    c = rnn_case('gru', H, 2, 2, w_dtype)
    need = 2 * 3 * H * H * (4 if w_dtype == VC_F32 else 2)
    for give in (None, need - 1, 0):
        out = _run('gru', c['xproj'], c['wf'], c['wb'], 2, w_dtype, VC_F32, ws_bytes=give, expect=VC_ERR_WORKSPACE)
        assert bool(torch.isnan(out).all()), 'a refused call wrote the output'


def test_recurrences_refuse_bad_shapes_and_dtypes():
    lib = _lib()
    x, w, out = nans(4, 64, VC_F32), nans(4, 64, VC_F32), nans(4, 64, VC_F32)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    for H, T, n_seq, wd, od in ((0, 1, 1, 0, 0), (1025, 1, 1, 0, 0), (2, 0, 1, 0, 0), (2, 1, 0, 0, 0), (2, 1, 1, 2, 0), (2, 1, 1, 0, 2),
                                (2, 1, 1, -1, 0)):
        assert lib.vc_gru_bidir(p(x), p(w), p(w), wd, n_seq, T, H, p(out), od, p(ws), 1 << 16, _st()) == VC_ERR_INVALID, (H, T, n_seq, wd, od)
    for H, T, n_seq, wd, od in ((0, 1, 1, 0, 0), (513, 1, 1, 0, 0), (2, 0, 1, 0, 0), (2, 1, 0, 0, 0), (2, 1, 1, 2, 0), (2, 1, 1, 0, 2)):
        assert lib.vc_lstm_bidir(p(x), p(w), p(w), wd, n_seq, T, H, p(out), od, _st()) == VC_ERR_INVALID, (H, T, n_seq, wd, od)
    assert lib.vc_gru_bidir(None, p(w), p(w), 0, 1, 1, 2, p(out), 0, p(ws), 1 << 16, _st()) == VC_ERR_INVALID
    assert int(lib.vc_gru_workspace_bytes(0, 0)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------ softmax + argmax

def _softmax(x, N, ldp, out_dtype, want_class=True, dual_ldp=None):
    """x [M, ldl] numpy (padding included) -> (probabilities tensor [M, ldp], class ids numpy or None[, bf16 copy])."""
    lib = _lib()
    M, ldl = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    prob = nans(M + 1, ldp, out_dtype)
    cls = torch.full((M + 1,), -77, dtype=torch.int32, device='cuda') if want_class else None
    if dual_ldp is None:
        _check(lib.vc_softmax_argmax(p(xd), M, N, ldl, p(prob), ldp, out_dtype, p(cls), _st()))
        second = None
    else:
        second = nans(M + 1, dual_ldp, VC_BF16)
        _check(lib.vc_softmax_argmax_dual(p(xd), M, N, ldl, p(prob), ldp, p(second), dual_ldp, p(cls), _st()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(second[M:].float()).all())
        second = second[:M]
    torch.cuda.synchronize()
    assert bool(torch.isnan(prob[M:].float()).all()), 'wrote past the last row'
    if cls is not None:
        assert int(cls[M]) == -77
        cls = cls[:M].cpu().numpy().astype(np.int64)
    return (prob[:M], cls) if dual_ldp is None else (prob[:M], cls, second)


def _softmax_bound(x):
    """8 x the float32 restatement's distance from float64 on this input, at least 1e-6."""
    want, cls = R.softmax_argmax(x)
    return want, cls, max(8.0 * float(np.abs(R.softmax_f32(x) - want).max()), 1e-6)


@pytest.mark.parametrize('N', SOFTMAX_N)
@pytest.mark.parametrize('M', SOFTMAX_M)
def test_softmax_argmax_against_float64(M, N):
    """Four rows per block (M = 1 .. 9), N on both sides of the 64-lane stride; ldl > N with NaN in the logits' padding;
    ldp > N must come back exactly zero; float32 probabilities against float64 and summing to 1 within the roundings
    of the row sum ((ceil(N / 64) + 9) 2^-24: the exponentials cancel between numerator and denominator); the bf16
    output is to_bf16 of the float32 output bit for bit; the dual form is the two single calls bit for bit;
    d_class = NULL is accepted."""
    poison_gpu_state()
    ldl, ldp, ldp2 = N + 3, N + 5, ((N + 7) // 8) * 8 + 8
    x = softmax_logits(M, N, ldl, 100 * M + N)
    want, want_cls, bound = _softmax_bound(x[:, :N])
    pf, cls = _softmax(x, N, ldp, VC_F32)
    got = val(pf)
    assert np.array_equal(cls, want_cls)
    assert bool((got[:, N:] == 0).all()) and not np.signbit(got[:, N:]).any()
    err = float(np.abs(got[:, :N] - want).max())
    print('MEASURED softmax M=%d N=%d err=%.2e bound=%.2e sum-1=%.2e' % (M, N, err, bound, float(np.abs(got[:, :N].sum(1) - 1).max())))
    assert err <= bound <= 5e-5
    assert float(np.abs(got[:, :N].sum(1) - 1.0).max()) <= ((N + 63) // 64 + 9) * 2.0 ** -24
    pb, cls_b = _softmax(x, N, ldp2, VC_BF16)
    assert np.array_equal(cls_b, want_cls)
    want_bits = np.zeros((M, ldp2), np.uint16)
    want_bits[:, :N] = R.to_bf16_bits(got[:, :N].astype(np.float32))
    assert np.array_equal(raw(pb).view(np.uint16), want_bits)
    d32, dcls, d16 = _softmax(x, N, ldp, VC_F32, dual_ldp=ldp2)
    assert np.array_equal(raw(d32), raw(pf)) and np.array_equal(raw(d16), raw(pb)) and np.array_equal(dcls, want_cls)
    p_nocls, none = _softmax(x, N, ldp, VC_F32, want_class=False)
    assert none is None and np.array_equal(raw(p_nocls), raw(pf))
    d32n, _, d16n = _softmax(x, N, ldp, VC_F32, want_class=False, dual_ldp=ldp2)
    assert np.array_equal(raw(d32n), raw(pf)) and np.array_equal(raw(d16n), raw(pb))
    poison_gpu_state()
    assert np.array_equal(raw(_softmax(x, N, ldp, VC_F32)[0]), raw(pf))


def test_softmax_argmax_ties_resolve_to_the_lowest_index():
    """Equal maxima inside one lane's stride (columns c and c + 64), in different lanes, and both at once (the lower
    index held by the higher lane): the class is the first maximum every time, in every row of a block."""
    for N, cols, first in SOFTMAX_TIES:
        x = softmax_logits(5, N, N + 1, N)
        x[:, :N] = np.round(x[:, :N])                       # integers: more exact ties below the maximum
        x[:, list(cols)] = 50.0
        x[4, :N] = 7.0                                      # a whole row of equal logits
        want, want_cls, bound = _softmax_bound(x[:, :N])
        assert list(want_cls) == [first] * 4 + [0]
        pf, cls = _softmax(x, N, N, VC_F32)
        assert list(cls) == list(want_cls), (N, cols, list(cls))
        assert float(np.abs(val(pf) - want).max()) <= bound


def test_softmax_argmax_large_logits():
    """Logits of +-1e4, differences far past where expf underflows, and a maximum shared by near neighbours."""
    N = 129
    x = np.full((6, N + 2), np.nan, np.float32)
    x[:, :N] = -1e4
    x[0, 17] = 1e4
    x[1, [3, 70, 128]] = 1e4
    x[1, 70] = 1e4 - 0.5
    x[2, :N] = 1e4 - 0.25 * np.arange(N)
    x[3, :N] = -1e4 + 0.25 * np.arange(N)
    x[4, :N] = np.where(np.arange(N) % 2 == 0, 1e4, -1e4)
    x[5, 128] = -1e4 + 1.0
    want, want_cls, bound = _softmax_bound(x[:, :N])
    pf, cls = _softmax(x, N, N, VC_F32)
    got = val(pf)
    err = float(np.abs(got - want).max())
    print('MEASURED softmax large logits err=%.2e bound=%.2e' % (err, bound))
    assert np.array_equal(cls, want_cls) and err <= bound <= 5e-5
    assert float(np.abs(got.sum(1) - 1.0).max()) <= 12 * 2.0 ** -24


@pytest.mark.parametrize('N', [1, 63, 129])
def test_softmax_argmax_class_of_a_degenerate_row_is_in_range(N):
    """A row of all -inf, all lowest-float or all NaN: no logit is > -FLT_MAX, and the kernel returned 0x7fffffff as its
    class.  The class must be 0 (tf.argmax on an all-equal row); the other rows of the block are unaffected.  The
    probabilities of such a row (NaN, 1 / N, NaN: include/vc_hip.h) are not asserted."""
    lo = np.finfo(np.float32).min
    x = softmax_logits(7, N, N + 1, N)
    x[1, :N], x[3, :N], x[4, :N] = -np.inf, lo, np.nan
    good = [0, 2, 5, 6]
    want, want_cls, bound = _softmax_bound(x[good, :N])
    for dual in (None, N + 3):
        r = _softmax(x, N, N + 2, VC_F32, dual_ldp=dual)
        cls, got = r[1], val(r[0])
        print('MEASURED softmax degenerate N=%d classes=%s p(-inf)=%s p(lowest)=%s p(nan)=%s' % (N, list(cls[[1, 3, 4]]), got[1, 0], got[3, 0], got[4, 0]))
        assert bool(((cls >= 0) & (cls < N)).all()), list(cls)
        assert list(cls[[1, 3, 4]]) == [0, 0, 0]
        assert np.array_equal(cls[good], want_cls) and float(np.abs(got[good, :N] - want).max()) <= bound
        assert bool((got[:, N:] == 0).all())


def test_softmax_argmax_refuses_bad_shapes():
    lib = _lib()
    x, out = nans(4, 8, VC_F32), nans(4, 8, VC_F32)
    for M, N, ldl, ldp, od in ((0, 4, 8, 8, 0), (4, 0, 8, 8, 0), (4, 8, 7, 8, 0), (4, 8, 8, 7, 0), (4, 8, 8, 8, 2)):
        assert lib.vc_softmax_argmax(p(x), M, N, ldl, p(out), ldp, od, None, _st()) == VC_ERR_INVALID
    assert lib.vc_softmax_argmax_dual(p(x), 4, 8, 8, p(out), 8, p(out), 7, None, _st()) == VC_ERR_INVALID
    assert lib.vc_softmax_argmax(None, 4, 8, 8, p(out), 8, 0, None, _st()) == VC_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------ conversion

def _convert(src_bits, sdt, ddt, n=None):
    """src_bits: numpy uint32 (float32) or uint16 (bf16) -> the destination's bits, canary after the n-th element checked."""
    lib = _lib()
    n = len(src_bits) if n is None else n
    s = torch.from_numpy(src_bits.view(np.int32 if sdt == VC_F32 else np.int16).copy()).cuda() if len(src_bits) else torch.zeros(1, dtype=torch.int32, device='cuda')
    fill = 0x5a5a5a5a if ddt == VC_F32 else 0x5a5a
    d = torch.full((n + 3,), fill, dtype=torch.int32 if ddt == VC_F32 else torch.int16, device='cuda')
    _check(lib.vc_convert(p(s), sdt, p(d), ddt, n, _st()))
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    assert bool((out[n:] == fill).all()), 'wrote past the n-th element'
    return out[:n].view(np.uint32 if ddt == VC_F32 else np.uint16)


@pytest.mark.parametrize('n', CONVERT_N)
def test_convert_lengths_and_dtype_pairs(n):
    """n = 0, one element, around one block, past the 4,096-block grid cap; all four dtype pairs: the same-dtype pairs
    copy, float32 -> bf16 rounds to nearest even (rnn_ref.to_bf16_bits), bf16 -> float32 is exact."""
    rng = np.random.RandomState(n % 1000)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    b32 = x.view(np.uint32)
    b16 = R.to_bf16_bits(x)
    assert np.array_equal(_convert(b32, VC_F32, VC_F32), b32)
    assert np.array_equal(_convert(b16, VC_BF16, VC_BF16), b16)
    assert np.array_equal(_convert(b32, VC_F32, VC_BF16), b16)
    assert np.array_equal(_convert(b16, VC_BF16, VC_F32), b16.astype(np.uint32) << 16)


def test_convert_rounding_edges():
    """Halfway cases in both parities, the largest finite values (the first that rounds to inf), +-0, +-inf: bit-exact
    against to_bf16_bits; NaN stays NaN; every bf16 pattern (NaNs apart) converts to float32 exactly."""
    ok, nan = convert_specials()
    assert np.array_equal(_convert(ok, VC_F32, VC_BF16), R.to_bf16_bits(ok.view(np.float32)))
    got = _convert(nan, VC_F32, VC_BF16)
    assert bool(np.isnan(R.from_bf16_bits(got)).all())
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    isnan = np.isnan(R.from_bf16_bits(every))
    wide = _convert(every, VC_BF16, VC_F32)
    assert np.array_equal(wide[~isnan], every[~isnan].astype(np.uint32) << 16) and bool(np.isnan(wide[isnan].view(np.float32)).all())
    back = _convert(wide, VC_F32, VC_BF16)
    assert np.array_equal(back[~isnan], every[~isnan])


def test_convert_preserves_subnormals():
    """float32 subnormals round to bf16 subnormals (nearest even) as torch does, and bf16 subnormals widen exactly."""
    sub = convert_subnormals()
    got = _convert(sub, VC_F32, VC_BF16)
    print('MEASURED convert subnormals f32->bf16 got=%s want=%s' % ([hex(v) for v in got], [hex(v) for v in R.to_bf16_bits(sub.view(np.float32))]))
    assert np.array_equal(got, R.to_bf16_bits(sub.view(np.float32)))
    assert np.array_equal(_convert(sub, VC_F32, VC_F32), sub)


def test_convert_refuses_bad_arguments():
    lib = _lib()
    a = nans(1, 8, VC_F32)
    assert lib.vc_convert(p(a), 2, p(a), 0, 8, _st()) == VC_ERR_INVALID and lib.vc_convert(p(a), 0, p(a), -1, 8, _st()) == VC_ERR_INVALID
    assert lib.vc_convert(None, 0, p(a), 0, 8, _st()) == VC_ERR_INVALID and lib.vc_convert(p(a), 0, None, 0, 8, _st()) == VC_ERR_INVALID
