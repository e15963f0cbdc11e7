"""The float64 definitions of tests/rnn_ref.py checked on the CPU against independent statements of the same operations
(oracle/model_oracle.py, torch.nn.LSTM, torch's bf16 conversion), and the input builders and shape tables of
tests/test_rnn_kernels_gpu.py proved usable before a device sees them: on every GPU input case each float32
restatement stays within the suite's 3e-2 (bf16) / 5e-5 (float32) of float64, and every bound the GPU file derives
stays below those figures."""
import functools

import numpy as np
import pytest
import torch

import rnn_ref as R

VC_F32, VC_BF16 = 0, 1
CAP = {True: 3e-2, False: 5e-5}          # today's flat tolerances: anything bf16 / float32 throughout
K_F32, K_BF16_STATE, FLOOR = 8.0, 4.0, 1e-6
BF16_STEP = 2.0 ** -8                    # one bf16 rounding of v moves it by at most 2^-8 |v|

# ------------------------------------------------------------------------------------------ host logic, restated

LDS_LIMIT = 150 * 1024


def gru_weights_in_lds(H, w_dtype):
    """vc_gru_bidir: h, r h, u (3 H floats) and the [H, 3H] weights in at most 150 KiB of LDS."""
    return 3 * H * 4 + 3 * H * H * (4 if w_dtype == VC_F32 else 2) <= LDS_LIMIT


def lstm_weights_in_lds(H, w_dtype):
    """vc_lstm_bidir: h and z (5 H floats) and the [H, 4H] weights."""
    return 5 * H * 4 + 4 * H * H * (4 if w_dtype == VC_F32 else 2) <= LDS_LIMIT


def gru_kernel(H, w_dtype, n_seq, gru_mfma=-1):
    """Which kernel vc_gru_bidir launches."""
    valu = (gru_mfma != 1) if gru_mfma >= 0 else (n_seq < 32)
    if w_dtype == VC_BF16 and H in (128, 256):
        return 'resident' if valu else 'mfma'
    if w_dtype == VC_F32 and H == 128:
        return 'resident'
    return 'wave' if H == 40 else 'generic'


def gru_bf16_state(kernel, w_dtype):
    """h and r h rounded to bf16 in front of the matrix products?"""
    return kernel == 'mfma' or (kernel == 'resident' and w_dtype == VC_BF16)


def generic_geometry(H):
    """(threads, KS1, KS2) of gru_generic_kernel."""
    nt = 256
    while nt < 512 and nt < 2 * H:
        nt *= 2
    ks1 = ks2 = 1
    while ks1 * 2 <= 64 and ks1 * 2 * 2 * H <= nt:
        ks1 *= 2
    while ks2 * 2 <= 64 and ks2 * 2 * H <= nt:
        ks2 *= 2
    return nt, ks1, ks2


def generic_columns(H, loops):
    """Gate and candidate columns gru_generic_kernel's thread groups compute when a group takes `loops` = (gate,
    candidate) columns, a group stride apart (1, 1: the kernel as it was)."""
    nt, ks1, ks2 = generic_geometry(H)
    g = {c + i * (nt // ks1) for c in range(nt // ks1) for i in range(loops[0])}
    c = {c + i * (nt // ks2) for c in range(nt // ks2) for i in range(loops[1])}
    return {x for x in g if x < 2 * H}, {x for x in c if x < H}


# ------------------------------------------------------------------------------------------ inputs

def _grid(a, w_dtype):
    a = np.asarray(a, np.float32)
    return R.to_bf16(a) if w_dtype == VC_BF16 else a


def _chequer(rows, cols, amp, shift=0):
    t, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return np.where((t + c // (1 + shift) + shift) % 2 == 0, amp, -amp).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rnn_case(cell, H, T, n_seq, w_dtype, kind='random', amp=40.0):
    """One input case, its float64 result and its restatements' distances from it.  cell 'gru' / 'lstm'; kind 'random':
    xproj ~ N(0, 1), weights ~ N(0, 1 / H) (a recurrent product of order 1), different in each direction;
    'saturated': gate columns at +-amp in a chequerboard over (frame, column), candidate (GRU) / j (LSTM) columns at
    +-amp in a coarser one, so the gates are 0 or 1 and the candidates -1 or 1 to float32 precision.
    Weights are on the bf16 grid when w_dtype is bf16: the float64 result is that of the numbers the device is given."""
    G = 3 if cell == 'gru' else 4
    rng = np.random.RandomState(1000 * G + 7 * H + 31 * T + n_seq + 2 * w_dtype + (500 if kind != 'random' else 0))
    rows = n_seq * T
    s = 1.0 / np.sqrt(H)
    wf, wb = (_grid(rng.standard_normal((H, G * H)) * s, w_dtype) for _ in range(2))
    if kind == 'random':
        xp = rng.standard_normal((rows, 2 * G * H)).astype(np.float32)
    else:
        halves = []
        for d in range(2):
            if cell == 'gru':
                halves += [_chequer(rows, 2 * H, amp, d), _chequer(rows, H, amp, 1 - d) * np.float32(-1 if d else 1)]
            else:
                halves += [_chequer(rows, H, amp, d), _chequer(rows, H, amp, 1), _chequer(rows, 2 * H, amp, 1 - d)]
        xp = np.concatenate(halves, axis=1)
        assert xp.shape == (rows, 2 * G * H)
    for a in (xp, wf, wb):
        a.setflags(write=False)
    if cell == 'gru':
        want = R.gru_bidir(xp, wf, wb, T)
        err = {False: float(np.abs(R.gru_bidir_f32(xp, wf, wb, T) - want).max()),
               True: float(np.abs(R.gru_bidir_f32(xp, wf, wb, T, bf16_state=True) - want).max())}
    else:
        want = R.lstm_bidir(xp, wf, wb, T)
        err = {False: float(np.abs(R.lstm_bidir_f32(xp, wf, wb, T) - want).max())}
    want.setflags(write=False)
    return dict(cell=cell, H=H, T=T, n_seq=n_seq, w_dtype=w_dtype, kind=kind, xproj=xp, wf=wf, wb=wb, want=want, err=err)


def rnn_bound(case, bf16_state, out_dtype):
    """(bound per element, the flat figure it must stay under).  k x the restatement's distance from float64 on this
    input (k = 8 float32 arithmetic, 4 where the restatement already holds the kernel's bf16 roundings), at least
    1e-6, plus one bf16 rounding of the expected value when the output is bf16."""
    k = K_BF16_STATE if bf16_state else K_F32
    b = np.full(case['want'].shape, max(k * case['err'][bf16_state], FLOOR))
    if out_dtype == VC_BF16:
        b = b + BF16_STEP * np.abs(case['want'])
    return b, CAP[bf16_state or out_dtype == VC_BF16 or case['w_dtype'] == VC_BF16]


def _rows(H, Ts, n, w, kinds=('random',)):
    return [(H, T, n if T == Ts[-1] else 1 + (n > 1), w, kind) for kind in kinds for T in (Ts if kind == 'random' else Ts[-1:])]


BOTH = (VC_F32, VC_BF16)
SAT = ('random', 'saturated', 'saturated100')
GENERIC_H = (1, 24, 64, 65, 112, 113, 128, 129, 159, 160, 256, 257, 300, 512, 513, 1024)
# group -> (gru_mfma option, [(H, T, n_seq, w_dtype, kind)]); T = 1 and 2 are the prefetch edges
GRU_GROUPS = {}
for _H in GENERIC_H:
    for _w in BOTH:
        GRU_GROUPS['generic-H%d-%s' % (_H, 'bf16' if _w else 'f32')] = (-1, _rows(_H, (1, 2, 7) if _H <= 256 else (1, 2, 4), 3 if _H <= 256 else 2, _w, SAT))
for _w in BOTH:
    GRU_GROUPS['wave-H40-%s' % ('bf16' if _w else 'f32')] = (
        -1, _rows(40, (1, 2, 11), 5, _w, SAT) + [(40, 6, n, _w, 'random') for n in (1, 4, 9)])
for _H, _w, _gm in ((128, VC_BF16, 0), (256, VC_BF16, 0), (128, VC_F32, -1)):
    GRU_GROUPS['resident-H%d-%s' % (_H, 'bf16' if _w else 'f32')] = (_gm, _rows(_H, (1, 2, 9), 3, _w, SAT) + [(_H, 5, 1, _w, 'random')])
for _H in (128, 256):
    GRU_GROUPS['mfma-H%d-bf16' % _H] = (1, _rows(_H, (1, 2, 6), 17, VC_BF16, SAT) + [(_H, 5, n, VC_BF16, 'random') for n in (1, 15, 16, 33)])
LSTM_H = (1, 40, 97, 98, 137, 138, 512)
LSTM_GROUPS = {'lstm-H%d-%s' % (_H, 'bf16' if _w else 'f32'): _rows(_H, (1, 2, 6), 3, _w, SAT) + [(_H, 4, 1, _w, 'random')]
               for _H in LSTM_H for _w in BOTH}
EXPECTED_GRU_KERNEL = {'generic-H128-f32': 'resident', 'generic-H128-bf16': 'resident', 'generic-H256-bf16': 'resident'}


def case_of(cell, row):
    H, T, n, w, kind = row
    amp = 100.0 if kind == 'saturated100' else 40.0
    return rnn_case(cell, H, T, n, w, 'random' if kind == 'random' else 'saturated', amp)


def softmax_logits(M, N, ldl, seed):
    """[M, ldl] float32, N(0, 3) logits, NaN in the padding columns."""
    x = np.full((M, ldl), np.nan, np.float32)
    x[:, :N] = np.random.RandomState(seed).standard_normal((M, N)) * 3.0
    return x


SOFTMAX_M, SOFTMAX_N = (1, 3, 4, 5, 9), (1, 61, 63, 64, 65, 129)
# (N, columns that share the maximum, the class that must win): within one lane's stride (c and c + 64), across lanes,
# across both (the lower index sits in the HIGHER lane)
SOFTMAX_TIES = [(129, (5, 69), 5), (129, (64, 128), 64), (65, (0, 64), 0), (63, (3, 7), 3), (129, (40, 41, 62), 40),
                (129, (9, 70), 9), (129, (3, 66), 3), (129, (66, 67, 3 + 64, 128), 66), (129, (1, 65, 2, 128), 1)]

CONVERT_N = (0, 1, 255, 256, 257, 4096 * 256 + 257)


def convert_specials():
    """float32 values where a float32 -> bf16 conversion can go wrong, as bits: halfway cases in both parities (and
    one bit to either side), the largest finite values (0x7f7f7fff stays finite, 0x7f7f8000 .. 0x7f7fffff round to
    inf), +-0, +-inf, NaNs, normals next to the subnormal range."""
    b = [0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001, 0x3f800000, 0x3fffffff,
         0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0x00000000, 0x7f800000, 0x00800000, 0x00808000, 0x00ff8000]
    b = b + [x | 0x80000000 for x in b]
    return np.array(b, np.uint32), np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7fa00000], np.uint32)


def convert_subnormals():
    """float32 subnormals (exact on the bf16 grid, halfway, odd) of both signs, as bits."""
    b = [0x00010000, 0x00018000, 0x00028000, 0x007f0000, 0x007fffff, 0x00008000, 0x00008001, 0x00000001, 0x00400000]
    return np.array(b + [x | 0x80000000 for x in b], np.uint32)


# ------------------------------------------------------------------------------------------ the reference against others

def _oracle_weights(rng, C, H):
    w = {}
    for d in ('fw', 'bw'):
        s = 'g/bidirectional_rnn/%s/gru_cell/' % d
        w[s + 'gates/kernel'] = torch.from_numpy(rng.standard_normal((C + H, 2 * H)) * 0.4)
        w[s + 'gates/bias'] = torch.from_numpy(rng.standard_normal(2 * H) * 0.4 + 1.0)
        w[s + 'candidate/kernel'] = torch.from_numpy(rng.standard_normal((C + H, H)) * 0.4)
        w[s + 'candidate/bias'] = torch.from_numpy(rng.standard_normal(H) * 0.4)
    return w


@pytest.mark.parametrize('N,T,C,H', [(1, 1, 3, 1), (3, 7, 5, 6), (2, 12, 9, 17)])
def test_gru_reference_equals_the_model_oracle(N, T, C, H):
    from oracle import model_oracle as mo
    rng = np.random.RandomState(N + T + C + H)
    w = _oracle_weights(rng, C, H)
    x = torch.from_numpy(rng.standard_normal((N, T, C)))
    want = mo.gru_bidirectional(x, w, 'g').numpy().reshape(N * T, 2 * H)
    xin, wh = [], []
    for d in ('fw', 'bw'):
        s = 'g/bidirectional_rnn/%s/gru_cell/' % d
        Wg, Wc = w[s + 'gates/kernel'].numpy(), w[s + 'candidate/kernel'].numpy()
        xin += [x.numpy().reshape(N * T, C) @ Wg[:C] + w[s + 'gates/bias'].numpy(),
                x.numpy().reshape(N * T, C) @ Wc[:C] + w[s + 'candidate/bias'].numpy()]
        wh.append(np.concatenate([Wg[C:], Wc[C:]], axis=1))
    got = R.gru_bidir(np.concatenate(xin, axis=1), wh[0], wh[1], T)
    assert got.shape == want.shape and float(np.abs(got - want).max()) < 1e-13


@pytest.mark.parametrize('N,T,C,H', [(1, 1, 3, 1), (3, 7, 5, 6), (2, 12, 9, 17)])
def test_lstm_reference_equals_torch_lstm(N, T, C, H):
    """torch.nn.LSTM orders its gates i, f, g, o and has no forget bias: ours are i, j (= g), f, o with +1 on f."""
    rng = np.random.RandomState(N + T + C + H)
    x = rng.standard_normal((N, T, C))
    lstm = torch.nn.LSTM(C, H, batch_first=True, bidirectional=True).double()
    xin, wh = [], []
    perm = np.concatenate([np.arange(H), 2 * H + np.arange(H), H + np.arange(H), 3 * H + np.arange(H)])   # ours -> torch's order
    for suffix in ('', '_reverse'):
        Wx, Wh, b = rng.standard_normal((C, 4 * H)) * 0.4, rng.standard_normal((H, 4 * H)) * 0.4, rng.standard_normal(4 * H) * 0.4
        bt = b.copy()
        bt[2 * H:3 * H] += 1.0
        with torch.no_grad():
            getattr(lstm, 'weight_ih_l0' + suffix).copy_(torch.from_numpy(Wx[:, perm].T.copy()))
            getattr(lstm, 'weight_hh_l0' + suffix).copy_(torch.from_numpy(Wh[:, perm].T.copy()))
            getattr(lstm, 'bias_ih_l0' + suffix).copy_(torch.from_numpy(bt[perm]))
            getattr(lstm, 'bias_hh_l0' + suffix).zero_()
        xin.append(x.reshape(N * T, C) @ Wx + b)
        wh.append(Wh)
    with torch.no_grad():
        want = lstm(torch.from_numpy(x))[0].numpy().reshape(N * T, 2 * H)
    got = R.lstm_bidir(np.concatenate(xin, axis=1), wh[0], wh[1], T)
    assert float(np.abs(got - want).max()) < 1e-13
    from oracle import model_oracle as mo
    w = {}
    for d, k in (('fw', 0), ('bw', 1)):
        # the oracle takes [x, h] W + b with W = [identity on the hoisted part; Wh]: feed xproj itself as x
        w['l/bidirectional_rnn/%s/lstm_cell/kernel' % d] = torch.from_numpy(np.concatenate([np.eye(4 * H), wh[k]], axis=0))
        w['l/bidirectional_rnn/%s/lstm_cell/bias' % d] = torch.zeros(4 * H, dtype=torch.float64)
    fw = mo.lstm_direction(torch.from_numpy(xin[0].reshape(N, T, 4 * H)), w, 'l/bidirectional_rnn/fw')
    bw = mo.lstm_direction(torch.from_numpy(xin[1].reshape(N, T, 4 * H)), w, 'l/bidirectional_rnn/bw', reverse=True)
    assert float(np.abs(got - torch.cat([fw, bw], 2).numpy().reshape(N * T, 2 * H)).max()) < 1e-13


def reversed_case(xp, wf, wb, T):
    """The input whose FORWARD half is the backward problem of (xp, wf, wb) and the other way round: frames reversed
    inside every sequence, direction halves of xproj and the two weight matrices swapped."""
    rows, W = xp.shape
    x = xp.reshape(rows // T, T, W)[:, ::-1]
    x = np.concatenate([x[..., W // 2:], x[..., :W // 2]], axis=2)
    return np.ascontiguousarray(x.reshape(rows, W)), wb, wf


def unreverse(y, T):
    """Maps the result of reversed_case back: equal to the original result."""
    rows, W = y.shape
    y = y.reshape(rows // T, T, W)[:, ::-1]
    return np.concatenate([y[..., W // 2:], y[..., :W // 2]], axis=2).reshape(rows, W)


@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_backward_half_is_the_forward_half_of_the_reversed_input(cell):
    c = rnn_case(cell, 17, 7, 3, VC_F32)
    f64, f32 = (R.gru_bidir, R.gru_bidir_f32) if cell == 'gru' else (R.lstm_bidir, R.lstm_bidir_f32)
    x2, wf2, wb2 = reversed_case(c['xproj'], c['wf'], c['wb'], c['T'])
    assert np.array_equal(unreverse(f64(x2, wf2, wb2, c['T']), c['T']), c['want'])
    assert np.array_equal(unreverse(f32(x2, wf2, wb2, c['T']), c['T']), f32(c['xproj'], c['wf'], c['wb'], c['T']))
    assert not np.array_equal(c['want'][:, :17], c['want'][:, 17:])


def test_to_bf16_equals_torch():
    ok, nan = convert_specials()
    rng = np.random.RandomState(3)
    bits = np.concatenate([ok, convert_subnormals(), rng.randint(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x).bfloat16()
    assert np.array_equal(R.to_bf16_bits(x).view(np.int16), want.view(torch.int16).numpy())
    assert np.array_equal(R.to_bf16(x).view(np.uint32), want.float().numpy().view(np.uint32))
    assert np.isnan(R.to_bf16(nan.view(np.float32))).all() and torch.isnan(torch.from_numpy(nan.view(np.float32)).bfloat16()).all()
    # by hand: ties to even in both parities, the first value that overflows, signed zeros
    hand = {0x3f808000: 0x3f80, 0x3f818000: 0x3f82, 0x3f808001: 0x3f81, 0x3f807fff: 0x3f80, 0x7f7f7fff: 0x7f7f,
            0x7f7f8000: 0x7f80, 0xff7f8000: 0xff80, 0x80000000: 0x8000, 0x00008000: 0x0000, 0x00018000: 0x0002}
    for k, v in hand.items():
        assert int(R.to_bf16_bits(np.array([k], np.uint32).view(np.float32))[0]) == v, hex(k)


def test_softmax_reference():
    x = softmax_logits(5, 129, 129, 1)
    p, c = R.softmax_argmax(x)
    pt = torch.softmax(torch.from_numpy(x).double(), -1).numpy()
    assert float(np.abs(p - pt).max()) < 1e-15 and np.array_equal(c, torch.from_numpy(x).double().argmax(-1).numpy())
    assert float(np.abs(R.softmax_f32(x) - p).max()) < 5e-7
    for N, cols, first in SOFTMAX_TIES:
        row = np.zeros((1, N))
        row[0, list(cols)] = 3.0
        assert min(cols) == first and int(R.softmax_argmax(row)[1][0]) == first


# ------------------------------------------------------------------------------------------ host logic

def test_weights_in_lds_thresholds():
    """The H on both sides of `base + wbytes <= 150 * 1024` that the GPU file runs."""
    assert [gru_weights_in_lds(H, VC_F32) for H in (112, 113)] == [True, False]
    assert [gru_weights_in_lds(H, VC_BF16) for H in (159, 160)] == [True, False]
    assert [lstm_weights_in_lds(H, VC_F32) for H in (97, 98)] == [True, False]
    assert [lstm_weights_in_lds(H, VC_BF16) for H in (137, 138)] == [True, False]
    assert max(H for H in range(1, 1025) if gru_weights_in_lds(H, VC_F32)) == 112
    assert max(H for H in range(1, 1025) if gru_weights_in_lds(H, VC_BF16)) == 159
    assert max(H for H in range(1, 513) if lstm_weights_in_lds(H, VC_F32)) == 97
    assert max(H for H in range(1, 513) if lstm_weights_in_lds(H, VC_BF16)) == 137
    assert {112, 113, 159, 160} <= set(GENERIC_H) and {97, 98, 137, 138} <= set(LSTM_H)


def test_generic_kernel_thread_map_covers_every_column():
    """One column per thread group (the kernel before it looped) leaves 768 of the 1,024 admitted sizes incomplete, the
    first H = 257; with up to 4 gate and 2 candidate columns per group every size is complete, and up to H = 256 a group
    still has exactly one column (the geometry of the shipped sizes is unchanged)."""
    bad = [H for H in range(1, 1025) if generic_columns(H, (1, 1)) != (set(range(2 * H)), set(range(H)))]
    assert len(bad) == 768 and bad[0] == 257
    for H in range(1, 1025):
        assert generic_columns(H, (4, 2)) == (set(range(2 * H)), set(range(H))), H
        nt, ks1, ks2 = generic_geometry(H)
        if H <= 256:
            assert nt // ks1 >= 2 * H and nt // ks2 >= H
    assert generic_geometry(1) == (256, 64, 64) and generic_geometry(64)[1] == 2 and generic_geometry(65)[1] == 1
    assert generic_geometry(128)[0] == 256 and generic_geometry(129)[0] == 512


def test_group_tables_reach_the_kernels_they_name():
    for name, (gm, rows) in GRU_GROUPS.items():
        kind = name.split('-')[0]
        for H, T, n, w, _ in rows:
            assert T <= 48 and n <= 40
            assert gru_kernel(H, w, n, gm) == EXPECTED_GRU_KERNEL.get(name, kind), (name, H, n)
    assert {r[2] for r in GRU_GROUPS['mfma-H256-bf16'][1]} >= {1, 15, 16, 17, 33}
    assert {r[2] for r in GRU_GROUPS['wave-H40-f32'][1]} >= {1, 4, 5, 9}
    assert gru_kernel(256, VC_BF16, 31) == 'resident' and gru_kernel(256, VC_BF16, 32) == 'mfma'


# ------------------------------------------------------------------------------------------ the GPU inputs are usable

def _all_rows():
    for name, (gm, rows) in GRU_GROUPS.items():
        for row in rows:
            yield 'gru', name, gm, row
    for name, rows in LSTM_GROUPS.items():
        for row in rows:
            yield 'lstm', name, -1, row


@pytest.mark.parametrize('cell', ['gru', 'lstm'])
def test_restatements_and_bounds_stay_under_the_flat_tolerances(cell):
    """On every GPU input case: each restatement (bf16 output included) within 3e-2 / 5e-5 of float64, every derived
    bound under the same figures, and the saturated cases saturate: |h| <= 1 with some |h| = 1 to float32 precision."""
    for cl, name, gm, row in _all_rows():
        if cl != cell:
            continue
        c = case_of(cell, row)
        states = (False,) if cell == 'lstm' else (gru_bf16_state(gru_kernel(c['H'], c['w_dtype'], c['n_seq'], gm), c['w_dtype']),)
        assert np.isfinite(c['want']).all() and float(np.abs(c['want']).max()) <= 1.0
        for st in states:
            assert c['err'][st] <= CAP[st or c['w_dtype'] == VC_BF16], (name, row, c['err'])
            assert st or c['err'][st] <= 5e-6, (name, row, c['err'])          # float32 state: rounding noise only
            for od in BOTH:
                b, cap = rnn_bound(c, st, od)
                assert float(b.max()) <= cap, (name, row, od, float(b.max()), cap)
            f32 = R.gru_bidir_f32 if cell == 'gru' else R.lstm_bidir_f32
            kw = dict(bf16_state=st) if cell == 'gru' else {}
            e = float(np.abs(f32(c['xproj'], c['wf'], c['wb'], c['T'], out_bf16=True, **kw) - c['want']).max())
            assert e <= CAP[True], (name, row, e)
        if cell == 'gru' and row[4] != 'random' and c['T'] > 1:
            assert float(np.abs(c['want']).max()) > 1.0 - 1e-6, (name, row)
