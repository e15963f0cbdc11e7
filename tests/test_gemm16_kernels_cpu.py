"""What tests/test_gemm16_kernels_gpu.py relies on, proven without a device: tests/gemm16_ref.py on its own split planes is
a float64 conv1d(padding='same') to 2^-21 (forward, data gradient, the ragged sum over the banks, and the filter
gradients with the pair tables of gemm16.bank_wgrad / conv3_wgrad restated, against torch.autograd); the exact cases of
tests/gemm16_cases.py are exactly representable, reach the launcher branch they are listed for (the launcher's rules
restated in gemm16_ref with the lines of vc_gemm16.hip quoted there), and see every layout mix-up."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm16_cases as Cs
import gemm16_ref as R

SPLIT_REL = 2.0 ** -21          # two operands, each split to 2^-22 of itself


def _conv_same64(x, W, pad_l=None):
    """x [N, T, cin] float64, W [k, cin, cout] (TF layout) -> [N, T, cout]; TF SAME: left pad (k - 1) // 2."""
    k = W.shape[0]
    pl = (k - 1) // 2 if pad_l is None else pad_l
    xp = F.pad(x.transpose(1, 2), (pl, k - 1 - pl))
    return F.conv1d(xp, W.permute(2, 1, 0)).transpose(1, 2)


def _rand(rng, *shape):
    """float32 values over several decades, row by row."""
    return (rng.standard_normal(shape) * np.exp(2.0 * rng.standard_normal(shape[:-1] + (1,)))).astype(np.float32)


def _forward_operand(W, n_groups_before=0):
    """W [k, cin, 128] -> (Bt [128, k * 2 cin] float16, col_scale [128]) by the reference vc_weights16, mode 0."""
    k, cin, _ = W.shape
    it = dict(src=W, dst='B', k=k, cin=cin, cout=128, mode=0, row_len=k * 2 * cin, tap_stride=2 * cin, plane_stride=cin, base=0, group=0,
              scale_dst='S', scale_off=0, scale_n=128)
    b = R.weights16([it], dict(B=np.full(128 * k * 2 * cin, np.nan, np.float16), S=np.zeros(128, np.float32)), 1)
    assert not np.isnan(b['B']).any()
    return b['B'].reshape(128, -1), b['S']


def _desc(X16, rs, M, T, Cn, pairs, ldc, cs, nbuf=None, **kw):
    d = dict(M=M, T=T, C=Cn, ldx=X16.shape[1], X16=X16, row_scale=rs, col_scale=cs, col_shift=None, pairs=pairs, ldc=ldc, ragged=0,
             accumulate=0, act=0, atomic_splits=0, nbuf=M * ldc if nbuf is None else nbuf)
    d.update(kw)
    return d


def _pair(Bt0, Bt1, taps0, extra, pad_l, c0, c1, row0=0, n0=0, n1=0, s0=0, s1=0):
    return dict(Bt0=Bt0, Bt1=Bt1, taps0=taps0, extra=extra, pad_l=pad_l, c_off0=c0, c_off1=c1, row0=row0, nrows0=n0, nrows1=n1, s_off0=s0, s_off1=s1)


def _close(got, ref, mag, what):
    e = np.abs(np.asarray(got) - np.asarray(ref)) / np.asarray(mag)
    assert e.max() <= SPLIT_REL, (what, float(e.max()))


# ------------------------------------------------------------------------------------------ the reference itself

def test_reference_forward_and_data_gradient_are_conv_same():
    rng = np.random.RandomState(1)
    N, T, Cn = 3, 10, 64
    M = N * T
    x = _rand(rng, M, Cn)
    W0, W1 = _rand(rng, 4, Cn, 128) * 0.1, _rand(rng, 5, Cn, 128) * 0.1
    x16, rs = R.split16(x, Cn, T)
    (B0, s0), (B1, s1) = _forward_operand(W0), _forward_operand(W1)
    out = R.gemm16(_desc(x16, rs, M, T, Cn, [_pair(B0, B1, 4, 1, 1, 0, 128)], 256, np.concatenate([s0, s1]))).reshape(M, 256)
    xt = torch.from_numpy(x.astype(np.float64)).view(N, T, Cn).requires_grad_(True)
    Wt = [torch.from_numpy(W.astype(np.float64)).requires_grad_(True) for W in (W0, W1)]
    y = torch.cat([_conv_same64(xt, Wt[0], 1), _conv_same64(xt, Wt[1], 1)], dim=2)
    mag = torch.cat([_conv_same64(xt.abs(), Wt[0].abs(), 1), _conv_same64(xt.abs(), Wt[1].abs(), 1)], dim=2).detach().numpy().reshape(M, 256)
    _close(out, y.detach().numpy().reshape(M, 256), mag, 'forward')
    # data gradient: dY [M, 128] convolved with the taps reversed (mode 1), left padding k - 1 - pad_l
    dy = _rand(rng, M, 128)
    (gx,) = torch.autograd.grad(_conv_same64(xt, Wt[1], 2), xt, torch.from_numpy(dy.astype(np.float64)).view(N, T, 128))
    k = 5
    it = dict(src=W1, dst='B', k=k, cin=Cn, cout=128, mode=1, row_len=k * 256, tap_stride=256, plane_stride=128, base=0, group=0,
              scale_dst='S', scale_off=0, scale_n=Cn)
    b = R.weights16([it], dict(B=np.full(Cn * k * 256, np.nan, np.float16), S=np.zeros(Cn, np.float32)), 1)
    Bt = np.zeros((128, k * 256), np.float16)
    Bt[:Cn] = b['B'].reshape(Cn, -1)
    d16, drs = R.split16(dy, 128, T)
    cs = np.ones(128, np.float32)
    cs[:Cn] = b['S']
    got = R.gemm16(_desc(d16, drs, M, T, 128, [_pair(Bt, None, k, 0, k - 1 - 2, 0, 0, n1=-1)], 128, cs)).reshape(M, 128)[:, :Cn]
    magx = _conv_same64(torch.from_numpy(np.abs(dy).astype(np.float64)).view(N, T, 128), Wt[1].detach().abs().flip(0).transpose(1, 2), k - 1 - 2)
    _close(got, gx.numpy().reshape(M, Cn), magx.numpy().reshape(M, Cn), 'data gradient')


def test_reference_ragged_walk_is_the_sum_over_the_banks():
    rng = np.random.RandomState(2)
    N, T, K, H = 2, 7, 4, 128
    M, Cn = N * T, 128 * K
    Ws = [_rand(rng, k, H, 128) * 0.1 for k in range(1, K + 1)]
    dz = _rand(rng, M, Cn)
    x = torch.zeros(N, T, H, dtype=torch.float64, requires_grad=True)
    z = torch.cat([_conv_same64(x, torch.from_numpy(W.astype(np.float64))) for W in Ws], dim=2)
    (ref,) = torch.autograd.grad(z, x, torch.from_numpy(dz.astype(np.float64)).view(N, T, Cn))
    PL = R.ragged_pl(Cn)
    items = [dict(src=W, dst='B', k=k, cin=H, cout=128, mode=1, row_len=2 * PL, tap_stride=128, plane_stride=PL, base=128 * k * (k - 1) // 2,
                  group=0, scale_dst='S' if k == 1 else None, scale_off=0, scale_n=H if k == 1 else 0) for k, W in enumerate(Ws, 1)]
    b = R.weights16(items, dict(B=np.full(H * 2 * PL, np.nan, np.float16), S=np.zeros(H, np.float32)), 1)
    assert not np.isnan(b['B']).any()
    d16, rs = R.split16(dz, Cn, T)
    d = _desc(d16, rs, M, T, Cn, [_pair(b['B'].reshape(H, -1), None, 0, 0, 0, 0, 0, n1=-1)], H, b['S'], ragged=1)
    mag = R.gemm16(dict(d, X16=np.abs(d16)), absolute=True).reshape(M, H)
    _close(R.gemm16(d).reshape(M, H), ref.numpy().reshape(M, H), mag, 'ragged walk')


def test_reference_weight_gradient_form_with_the_pair_tables_restated():
    """gemm16.bank_wgrad and gemm16.conv3_wgrad restated on the reference's own transposed operands, against autograd."""
    rng = np.random.RandomState(3)
    N, T, K, H = 4, 16, 4, 64
    M, CB = N * T, 128 * K
    x, dz = _rand(rng, M, H), _rand(rng, M, CB)
    Ws = [torch.zeros(k, H, 128, dtype=torch.float64, requires_grad=True) for k in range(1, K + 1)]
    xt = torch.from_numpy(x.astype(np.float64)).view(N, T, H)
    refs = torch.autograd.grad(torch.cat([_conv_same64(xt, W) for W in Ws], dim=2), Ws, torch.from_numpy(dz.astype(np.float64)).view(N, T, CB))
    shift0 = -(K // 2 - 1)
    XT, rsX = R.transpose_split16(x, H, T, shift0, K)
    ZT, rsZ = R.transpose_split16(dz, CB, T)
    sizes = [k * H * 128 for k in range(1, K + 1)]
    offs = 61 + np.concatenate([[0], np.cumsum(sizes)])
    pairs = []
    for p in range(K // 2):                               # gemm16.bank_wgrad: rows (shift, channel), frames contracted
        k0 = 2 * p + 1
        pairs.append(_pair(ZT[128 * (k0 - 1):128 * k0], ZT[128 * k0:128 * (k0 + 1)], 1, 0, 0, int(offs[k0 - 1]), int(offs[k0]),
                           row0=(-p - shift0) * H, n0=k0 * H, n1=(k0 + 1) * H, s0=128 * (k0 - 1), s1=128 * k0))
    rows = K * H
    d = _desc(XT, rsX, rows, rows, M, pairs, 128, rsZ, nbuf=int(offs[-1]) + 3, atomic_splits=2)
    got = R.gemm16(d)
    assert not got[:61].any() and not got[int(offs[-1]):].any()
    mag = R.gemm16(d, absolute=True)
    for k, rk in enumerate(refs, 1):
        sl = slice(int(offs[k - 1]), int(offs[k]))
        _close(got[sl], rk.numpy().ravel(), np.maximum(mag[sl], 1e-300), 'bank %d filter gradient' % k)
    # gemm16.conv3_wgrad: the small operand carries the shifts; tile [(shift, o), c], then dW[j] = tile[2 - j].T
    Hq = 128
    P, dq = _rand(rng, M, CB), _rand(rng, M, Hq)
    W1 = torch.zeros(3, CB, Hq, dtype=torch.float64, requires_grad=True)
    (ref1,) = torch.autograd.grad(_conv_same64(torch.from_numpy(P.astype(np.float64)).view(N, T, CB), W1), W1,
                                  torch.from_numpy(dq.astype(np.float64)).view(N, T, Hq))
    PT, rsP = R.transpose_split16(P, CB, T)
    QT, rsQ = R.transpose_split16(dq, Hq, T, -1, 3)
    pairs = [_pair(PT[256 * i:256 * i + 128], PT[256 * i + 128:256 * i + 256], 1, 0, 0, 256 * i, 256 * i + 128, n0=3 * Hq, n1=3 * Hq,
                   s0=256 * i, s1=256 * i + 128) for i in range(CB // 256)]
    d = _desc(QT, rsQ, 3 * Hq, 3 * Hq, M, pairs, CB, rsP, atomic_splits=5)
    got = np.flip(R.gemm16(d).reshape(3, Hq, CB), 0).transpose(0, 2, 1)
    mag = np.flip(R.gemm16(d, absolute=True).reshape(3, Hq, CB), 0).transpose(0, 2, 1)
    _close(got, ref1.numpy(), mag, 'projection filter gradient')


def test_bit_model_of_the_split():
    """x s = hi + lo to 2^-22 of itself (or float16's subnormal spacing), powers of two, largest hi in [2^14, 2^15]."""
    rng = np.random.RandomState(4)
    x = _rand(rng, 24, 64)
    x[5] = 0.0
    x16, rs = R.split16(x, 64, 6)
    rec = (x16[:, :64].astype(np.float64) + x16[:, 64:].astype(np.float64)) * rs[:, None]
    winmax = np.abs(x).reshape(4, -1).max(1).repeat(6)[:, None]
    assert (np.abs(rec - x) <= np.maximum(np.abs(x) * 2.0 ** -21.5, winmax * 2.0 ** -37)).all()
    assert (np.log2(rs) % 1 == 0).all() and (rs.reshape(4, 6) == rs.reshape(4, 6)[:, :1]).all()
    him = np.abs(x16[:, :64].astype(np.float64)).reshape(4, -1).max(1)
    assert ((him >= 2.0 ** 14) & (him <= 2.0 ** 15)).all()
    assert R.pow2_scale(np.float32(0)) == (1.0, 1.0) and R.pow2_scale(np.float32(np.inf)) == (1.0, 1.0) and R.pow2_scale(np.float32(np.nan)) == (1.0, 1.0)
    assert R.pow2_scale(np.float32(2.0 ** -140)) == (2.0 ** 114, 2.0 ** -114)        # the exponent clamp at -100
    assert R.pow2_scale(np.float32(3.0)) == (2.0 ** 13, 2.0 ** -13)


# ------------------------------------------------------------------------------------------ the cases

def test_exact_cases_are_exactly_representable():
    for name in Cs.EXACT:
        d = Cs.get(name)
        X = d['X16'][:, :2 * d['C']].astype(np.float64)
        xin = X[~np.isnan(X)]
        assert (xin == np.round(xin)).all() and np.isnan(d['X16'][:, 2 * d['C']:]).all(), name
        wmax = 0.0
        for p in d['pairs']:
            for B in (p['Bt0'], p['Bt1']):
                if B is not None:
                    B = B.astype(np.float64)
                    assert (B == np.round(B)).all(), name
                    wmax = max(wmax, np.abs(B).max())
        n = max(R.products_per_output(d, p, False) for p in d['pairs'])
        assert n * np.abs(xin).max() * wmax < 2.0 ** 24, (name, n)                   # sum |x| |w| over the three products
        for s in ('row_scale', 'col_scale'):
            if d[s] is not None:
                assert (d[s] > 0).all() and (np.log2(d[s]) % 1 == 0).all(), (name, s)
        ref = Cs.reference(name)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref, equal_nan=True), name + ': a result is no float32 number'
        m = R.stored_mask(d)
        assert np.isnan(ref[m]).sum() == (0 if not name.startswith('nan_') or name.endswith('_clean') else d['T'] * 128 * 2 * len(d['pairs'])), name
        assert (ref[~m] == (0.0 if d['atomic_splits'] else Cs.SENTINEL)).all() and (~m).any(), name


def test_cases_reach_the_launcher_branch_they_are_listed_for():
    seen = set()
    for name in Cs.EXACT:
        d = Cs.get(name)
        ws = {'full': R.workspace_bytes(d['M'], d['C'], len(d['pairs'])), 'small': 4096, 'none': 0}[d['ws']]
        plan = R.launch_plan(d, d['forced'], ws)
        assert d['expect'], name
        for k, v in d['expect'].items():
            assert plan[k] == v, (name, k, plan[k], v)
        seen.add((plan['form'], plan['ks'], plan['split_map'], plan['idle'] > 0, bool(d['ragged'])))
    forms = {s[0] for s in seen}
    assert forms == {'plain', 'split', 'xcd16', 'atomic'}
    assert {s[1] for s in seen if s[0] == 'split' and not s[4]} >= {2, 3, 4, 6, 8} and {s[1] for s in seen if s[4] and s[0] == 'split'} >= {3, 4, 8}
    assert ('split', 2, 1, True, False) in seen and ('split', 4, 1, True, False) in seen and ('split', 8, 1, False, False) in seen
    assert any(s[0] == 'xcd16' and s[3] for s in seen)                               # one half empty at one row tile
    # the rules themselves, at the values the issue quotes
    assert R.split_points(9, 3, 2, False) == [0, 5, 9] and R.choose_ksplit(260, 1, 9) == 2 and R.choose_ksplit(260, 2, 48) == 1
    assert R.choose_ksplit(1200, 1, 48) == 8 and R.choose_ksplit(256 * 100, 1, 48) == 2 and R.choose_ksplit(130, 1, 6) == 1
    assert R.split_points(12, 4, 3, True) == [0, 4, 8, 12] and R.split_points(18, 6, 4, True)[-1] == 18
    for ntm in (1, 2, 3):
        blocks, work = R.pair16_map(ntm)
        got = sorted(w for w in work if w is not None)
        assert got == sorted((p, rt) for p in range(16) for rt in range(ntm)), ntm   # every tile of every pair exactly once
    assert R.pair16_map(1)[0] == 32 and sum(w is None for w in R.pair16_map(1)[1]) == 16


def test_operand_cases_reach_their_paths():
    for name, M, T, Cn, ldx in Cs.SPLIT16_SHAPES:
        assert R.split16_tl_seg(M, Cn, T) == Cs.SPLIT16_TL[name], name
    assert {Cs.SPLIT16_TL[n][1] for n in Cs.SPLIT16_TL} >= {1, 3, 4, 5, 7}           # 5 and 7 groups: more than one pass of four
    assert Cs.SPLIT16_TL['w1100'][2] == 1 and 2200 // 2 > 1024
    # the prologue's fmaf is exact in float64: every product and sum below is a float64 number with bits to spare
    X, M, T, Cn, scale, shift = Cs.prologue_input()
    v = X.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    assert (v == np.round(v * 2) / 2).all() and np.abs(v).max() < 2.0 ** 20
    for name in [s[0] for s in Cs.TRANSPOSE]:
        X, M, T, Cn, ldx, s0, ns = Cs.transpose_input(name)
        assert M % 64 == 0 and M % T == 0 and s0 > -T and s0 + ns - 1 < T
    assert any(s[2] % 64 and s[6] > 1 for s in Cs.TRANSPOSE) and any(s[6] == 64 for s in Cs.TRANSPOSE)


# ------------------------------------------------------------------------------------------ layout mix-ups

@pytest.mark.parametrize('mix,name', [('swap_x_planes', 'rows260'), ('swap_w_planes', 'rows260'), ('lolo', 'rows260'), ('tap_neighbour', 'rows260'),
                                      ('pad_plus', 'rows260'), ('pad_minus', 'rows260'), ('first_extra_tap', 'rows260'),
                                      ('tap_neighbour', 'rag_4'), ('bank_neighbour', 'rag_4'), ('half_neighbour', 'rag_4'),
                                      ('s_off_for_c_off', 'atomic_z2')])
def test_a_layout_mix_up_changes_an_exact_reference(mix, name):
    d = Cs.get(name)
    m = R.stored_mask(d)
    assert (R.gemm16(d, mix=mix)[m] != Cs.reference(name)[m]).mean() > 0.2


def test_one_hot_cases_see_each_plane_product():
    """x_hi one-hot: the output is w_hi + w_lo of one tap; x_lo one-hot: w_hi alone (there is no lo * lo)."""
    for i, (f, c, pl) in enumerate(Cs.ONEHOT):
        d = Cs.get('onehot_%d' % i)
        out = Cs.reference('onehot_%d' % i)[:260 * 256].reshape(260, 256)
        W = d['pairs'][0]['Bt1'].astype(np.float64).reshape(128, 4, 2, 128)
        for m in range(max(f - 2, 0), min(f + 2, 259)):
            j = f - m + 1                                   # tap of the wider filter that reads frame f at row m
            want = 0.0
            if 0 <= j < 4 and m // 130 == f // 130:
                want = W[:, j, 0, c] + (W[:, j, 1, c] if pl == 0 else 0.0)
            assert np.array_equal(out[m, 128:], np.broadcast_to(want, 128)), (f, c, pl, m)


def test_operand_mix_ups_change_the_bit_model():
    X, M, T, Cn, ldx, s0, ns = Cs.transpose_input('t20_3')
    a, _ = R.transpose_split16(X, Cn, T, s0, ns)
    b, _ = R.transpose_split16(X, Cn, T, s0, ns, shift_bias=1)
    assert (a != b).mean() > 0.01
    items, bufs, n_groups = Cs.weights16_case('mode0')
    host = {k: np.zeros(n, dt) for k, (dt, n) in bufs.items()}
    a, b = R.weights16(items, host, n_groups), R.weights16(items, host, n_groups, mode_as=1)
    assert all((a[k] != b[k]).mean() > 0.2 for k in 'ABC')
