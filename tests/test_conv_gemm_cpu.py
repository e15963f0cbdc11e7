"""tests/conv_gemm_ref.py (the float64 definition of vc_gemm_desc) checked without a GPU -- against the oracle's blocks,
against float64 torch convolutions and autograd -- plus the host-only exports of vc_conv_gemm, and the soundness of
tests/conv_gemm_cases.py, the cases that tests/test_conv_gemm_gpu.py runs on the device.

Those cases hold small integers (X in [-3, 3], weights in {-2..2}, power-of-two scales, integer shifts and
residuals).  `exactness()` proves for every one of them what the device test leans on: sum |A| |B| -- an upper bound of
every partial sum in any order -- and every later intermediate stay below 2^24, so float32 arithmetic is exact in any
summation order, and every result stored as bf16 is an integer of magnitude <= 256 (or, for the highway gate's halves,
a multiple of 1/2 below 128), which bf16 holds exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_gemm_ref as R
from conv_gemm_cases import (DROPOUT_CASES, EXACT_CASES, FORMS, ISOLATION_CASES, ORDER_CASES, ZERO_CASES, case, cases_of, exactness,
                             expected_form, make_exact, make_order, make_zeros)
from conv_gemm_ref import ACT_NONE, ACT_RELU, BF16, F32, HIGHWAY, PLAIN
from oracle import model_oracle as mo

F64 = torch.float64


@pytest.mark.parametrize('form', FORMS)
def test_every_table_row_selects_its_kernel_form(form):
    rows = cases_of(form)
    assert rows, form
    for s in rows:
        assert expected_form(s) == form, (s.name, expected_form(s))
        for opt in s.toggle:
            if opt != 'proj256_split':
                assert expected_form(s, {opt: 0}) != form, (s.name, opt)
    if form not in ('conv256', 'bank256', 'proj256'):
        assert {s.dtype for s in rows} == {F32, BF16}, form


def test_every_isolation_row_selects_its_kernel_form():
    assert {s.form for s in ISOLATION_CASES} >= {'gemm_mi1', 'gemm_mi2', 'conv_kernel', 'conv256', 'bank256', 'proj256'}
    for s in ISOLATION_CASES:
        assert expected_form(s) == s.form, (s.name, expected_form(s))


def test_every_descriptor_field_is_non_default_in_some_exact_case():
    got = {k: set() for k in ('pro_affine', 'pro_relu', 'pro_pool', 'epi_scale', 'epi_shift', 'act', 'out_f32', 'sum_groups',
                              'epi_pool', 'mode', 'ws')}
    for s in EXACT_CASES:
        for k in got:
            got[k].add(getattr(s, k))
        assert s.ldx > s.Cin and s.ldc > (s.Cin if s.mode == HIGHWAY else s.N)
    assert got['pro_pool'] == {0, 1, 2} and got['sum_groups'] >= {0, 1, 2, 3} and got['mode'] == {PLAIN, HIGHWAY}
    assert got['ws'] >= {'full', 'none', 'small', 'misaligned'}
    for k in ('pro_affine', 'pro_relu', 'epi_scale', 'epi_shift', 'out_f32', 'epi_pool'):
        assert got[k] == {0, 1}, k
    assert any(s.ldr and s.ldr != s.N for s in EXACT_CASES) and any(p != (t - 1) // 2 for s in EXACT_CASES for p, t in zip(s.pad_l, s.taps))
    assert any(s.T == 1 for s in EXACT_CASES) and any(s.T < max(s.taps) for s in EXACT_CASES)
    assert any((c * 4) % 16 for s in EXACT_CASES for c in s.c_off if s.dtype == F32 and not s.sum_groups)


def _other_exact_cases():
    """The prologue-order, signed-zero and dropout cases, which the device test also compares exactly.  Dropout: the
    proof is of the value in front of the division by keep, which is one correctly rounded float32 operation."""
    out = [(s, make_order(s)) for s in ORDER_CASES] + [(s, make_zeros(s)) for s in ZERO_CASES]
    for s in DROPOUT_CASES:
        d = make_exact(s)
        d.drop_keep = 0.0
        out.append((s, d))
    return out


@pytest.mark.parametrize('form', FORMS + ('other',))
def test_exact_cases_stay_exactly_representable(form):
    if form == 'other':
        rows = _other_exact_cases()
        assert all(expected_form(s) == s.form for s, _ in rows)
    else:
        rows = [(s, make_exact(s)) for s in cases_of(form) + [s for s in ISOLATION_CASES if s.form == form]]
    for s, d in rows:
        big, stored, grid = exactness(s, d)
        big = big / s.drop_keep if s.drop_keep > 0 else big
        assert big < 2.0 ** 24, (s.name, big)
        assert grid, s.name
        if d.dtype == BF16 and not d.out_f32:
            assert stored <= (128.0 if d.mode == HIGHWAY else 256.0), (s.name, stored)
        else:
            assert stored < 2.0 ** 23, (s.name, stored)
        if d.dtype == BF16:
            # operands, and what the affine prologue re-rounds to bf16, are bf16 values already
            P = R.prologue(d.X[:, :d.Cin], d.T, d.pro_scale, d.pro_shift, d.pro_relu, 0)
            assert np.array_equal(R.bf16_round(P), P) and all(np.array_equal(R.bf16_round(g.W), g.W) for g in d.groups)


# ------------------------------------------------------------------------------------------ reference vs the oracle's blocks
def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=F64)


def _shapes(form, limit=6):
    """(N windows, T, Cin, N columns, taps) of the GPU table, a few per form."""
    seen, out = set(), []
    for s in cases_of(form):
        key = (s.T, s.Cin, s.N, s.taps)
        if key not in seen and s.M * max(s.taps) * s.Cin <= 1 << 20:
            seen.add(key)
            out.append(s)
    return out[:limit]


@pytest.mark.parametrize('form', ['gemm_mi1', 'conv_kernel', 'conv256'])
def test_reference_matches_oracle_conv1d_and_torch_conv1d(form):
    rng = np.random.RandomState(1)
    for s in _shapes(form):
        for g, taps in enumerate(s.taps):
            nw = s.M // s.T
            X = rng.standard_normal((s.M, s.Cin))
            k = rng.standard_normal((taps, s.Cin, s.N))                      # TF layout [taps, Cin, Cout]
            Bt = k.reshape(taps * s.Cin, s.N).T
            pad_l = (taps - 1) // 2
            got = R.conv_gemm(R.desc(X, s.T, s.N, [R.group(Bt, taps, pad_l, 0)]), round_out=False)
            want = mo.conv1d(_t(X).view(nw, s.T, s.Cin), _t(k)).reshape(s.M, s.N).numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), s.name
            # a left padding of the caller's choice: explicit zero padding in front of torch's convolution
            for pl in {0, taps - 1}:
                xp = torch.nn.functional.pad(_t(X).view(nw, s.T, s.Cin).transpose(1, 2), (pl, taps - 1 - pl))
                want = torch.nn.functional.conv1d(xp, _t(k).permute(2, 1, 0).contiguous()).transpose(1, 2).reshape(s.M, s.N).numpy()
                got = R.conv_gemm(R.desc(X, s.T, s.N, [R.group(Bt, taps, pl, 0)]), round_out=False)
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (s.name, pl)


def test_reference_matches_oracle_dense_bias_activation():
    rng = np.random.RandomState(2)
    for s in _shapes('gemm_mi1', 8):
        X, k, b = rng.standard_normal((s.M, s.Cin)), rng.standard_normal((s.Cin, s.N)), rng.standard_normal(s.N)
        w = {'d/kernel': _t(k), 'd/bias': _t(b)}
        for act, name in ((ACT_NONE, None), (ACT_RELU, 'relu'), (R.ACT_SIGMOID, 'sigmoid')):
            got = R.conv_gemm(R.desc(X, s.T, s.N, [R.group(k.T, 1, 0, 0)], epi_shift=b, act=act), round_out=False)
            assert np.abs(got - mo.dense(_t(X), w, 'd', name).numpy()).max() <= 1e-12 * s.Cin, s.name


def test_reference_matches_oracle_banks_bn_relu_pool():
    rng = np.random.RandomState(3)
    for s in _shapes('bank256', 4):
        K, nw, Cin = min(len(s.taps), 4), s.M // s.T, s.Cin
        X = rng.standard_normal((s.M, Cin))
        w = {}
        groups = []
        for k in range(1, K + 1):
            ker = rng.standard_normal((k, Cin, 128)) / np.sqrt(k * Cin)
            w['b/conv1d/conv1d/kernel' if k == 1 else 'b/num_%d/conv1d/conv1d/kernel' % k] = _t(ker)
            groups.append(R.group(ker.reshape(k * Cin, 128).T, k, (k - 1) // 2, 128 * (k - 1)))
        Cn = 128 * K
        bnw = {'gamma': rng.uniform(0.5, 2, Cn), 'beta': rng.standard_normal(Cn), 'moving_mean': rng.standard_normal(Cn) * 0.1,
               'moving_variance': rng.uniform(0.5, 2, Cn)}
        for kk, v in bnw.items():
            w['b/bn/' + kk] = _t(v)
        scale = bnw['gamma'] / np.sqrt(bnw['moving_variance'] + mo.BN_EPS)
        shift = bnw['beta'] - bnw['moving_mean'] * scale
        want = mo.conv1d_banks(_t(X).view(nw, s.T, Cin), w, 'b', K)
        d = R.desc(X, s.T, 128, groups, epi_scale=scale, epi_shift=shift, act=ACT_RELU)
        assert np.abs(R.conv_gemm(d, round_out=False) - want.reshape(s.M, Cn).numpy()).max() <= 1e-11, s.name
        # the pool as the producer's epilogue, and as the consumer's prologue (in front of a k = 3 convolution)
        pooled = mo.max_pool_2_same(want)
        d.epi_pool = 1
        assert np.abs(R.conv_gemm(d, round_out=False) - pooled.reshape(s.M, Cn).numpy()).max() <= 1e-11, s.name
        ker = rng.standard_normal((3, Cn, 16)) / np.sqrt(3 * Cn)
        for pp in (1, 2):
            got = R.conv_gemm(R.desc(want.reshape(s.M, Cn).numpy(), s.T, 16, [R.group(ker.reshape(3 * Cn, 16).T, 3, 1, 0)], pro_pool=pp),
                              round_out=False)
            assert np.abs(got - mo.conv1d(pooled, _t(ker)).reshape(s.M, 16).numpy()).max() <= 1e-11, s.name


def test_reference_prologue_is_bn_relu_pool_of_the_oracle_and_padding_stays_zero():
    rng = np.random.RandomState(4)
    nw, T, Cin, N = 3, 5, 8, 4
    X = rng.standard_normal((nw * T, Cin))
    w = {'bn/gamma': _t(rng.uniform(0.5, 2, Cin)), 'bn/beta': _t(rng.standard_normal(Cin) + 3.0),
         'bn/moving_mean': _t(rng.standard_normal(Cin)), 'bn/moving_variance': _t(rng.uniform(0.5, 2, Cin))}
    scale = (w['bn/gamma'] * torch.rsqrt(w['bn/moving_variance'] + mo.BN_EPS)).numpy()
    shift = w['bn/beta'].numpy() - w['bn/moving_mean'].numpy() * scale
    ker = rng.standard_normal((3, Cin, N))
    for relu in (0, 1):
        for pool in (0, 1):
            y = mo.bn(_t(X).view(nw, T, Cin), w, 'bn')
            y = torch.relu(y) if relu else y
            y = mo.max_pool_2_same(y) if pool else y
            want = mo.conv1d(y, _t(ker)).reshape(nw * T, N).numpy()       # F.pad zeros AFTER bn: padding is not shifted
            got = R.conv_gemm(R.desc(X, T, N, [R.group(ker.reshape(3 * Cin, N).T, 3, 1, 0)], pro_scale=scale, pro_shift=shift,
                                     pro_relu=relu, pro_pool=pool), round_out=False)
            assert np.abs(got - want).max() <= 1e-12 * 3 * Cin * 10, (relu, pool)


def test_reference_matches_oracle_highwaynet():
    rng = np.random.RandomState(5)
    for s in _shapes('highway_mi1', 8):
        H = s.Cin
        X = rng.standard_normal((s.M, H))
        W1, W2, b1, b2 = rng.standard_normal((H, H)), rng.standard_normal((H, H)), rng.standard_normal(H), rng.standard_normal(H)
        w = {'h/dense1/kernel': _t(W1), 'h/dense1/bias': _t(b1), 'h/dense2/kernel': _t(W2), 'h/dense2/bias': _t(b2)}
        Bt, sh = R.highway_pack(W1, b1, W2, b2)
        assert Bt.shape[0] == s.N == 64 * ((H + 31) // 32)
        d = R.desc(X, s.T, s.N, [R.group(Bt, 1, 0, 0)], mode=HIGHWAY, epi_shift=sh, ldc=s.ldc)
        got = R.conv_gemm(d, round_out=False)
        assert np.abs(got[:, :H] - mo.highwaynet(_t(X), w, 'h').numpy()).max() <= 1e-12 * H, s.name
        assert np.isnan(got[:, H:]).all()


def test_reference_sum_groups_is_the_autograd_data_gradient_of_the_banks():
    rng = np.random.RandomState(6)
    nw, T, Cin, F = 2, 7, 8, 4
    for K in (3, 4):
        x = _t(rng.standard_normal((nw, T, Cin))).requires_grad_(True)
        kers = [_t(rng.standard_normal((k, Cin, F))) for k in range(1, K + 1)]
        y = torch.cat([mo.conv1d(x, k) for k in kers], dim=-1)
        dZ = rng.standard_normal((nw * T, F * K))
        y.backward(_t(dZ).view(nw, T, F * K))
        groups = []
        for k, ker in zip(range(1, K + 1), kers):
            # dX = conv of dZ_k with the taps flipped and the kernel transposed: Bt[c, j * F + o] = W[k - 1 - j, c, o]
            Bt = ker.numpy()[::-1].transpose(1, 0, 2).reshape(Cin, k * F)
            groups.append(R.group(Bt, k, k - 1 - (k - 1) // 2, F * (k - 1)))
        for S in (1, 2):
            d = R.desc(dZ, T, Cin, groups, Cin=F, sum_groups=S)
            got = R.conv_gemm(d, C0=np.zeros((nw * T, Cin)) if S > 1 else None, round_out=False)
            assert np.abs(got - x.grad.reshape(nw * T, Cin).numpy()).max() <= 1e-12 * K * K * F, (K, S)


def test_reference_dropout_residual_order_and_storage_rounding():
    X = np.array([[1.0, 2.0], [3.0, -4.0]])
    W = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    Rr = np.full((2, 3), 10.0)
    d = R.desc(X, 1, 3, [R.group(W, 1, 0, 2)], epi_scale=np.array([9, 9, 2.0, 2.0, 2.0]), epi_shift=np.array([9, 9, 1.0, 1.0, 1.0]),
               act=ACT_RELU, R=Rr, ldc=7, drop_keep=0.25, drop_seed=5)
    keep = R.drop_mask(2, 7, 3, 5, 0.25, c_off=2)
    assert np.array_equal(keep, R.drop_mask(2, 7, 5, 5, 0.25)[:, 2:])         # the index is m * ldc + c_off + n
    want = np.maximum(np.array([[3.0, 5.0, 7.0], [7.0, -7.0, -1.0]]), 0.0) * 4.0 * keep + 10.0
    got = R.conv_gemm(d)
    assert np.array_equal(got[:, 2:5], want) and np.isnan(got[:, :2]).all() and np.isnan(got[:, 5:]).all()
    assert np.array_equal(R.bf16_round(np.array([1.00390625, 257.0, -0.0])), np.array([1.0, 256.0, 0.0]))
    assert R.conv_gemm(R.desc(np.array([[257.0]]), 1, 1, [R.group([[1.0]], 1, 0, 0)], dtype=BF16))[0, 0] == 256.0
    assert R.conv_gemm(R.desc(np.array([[257.0]]), 1, 1, [R.group([[1.0]], 1, 0, 0)], dtype=BF16, out_f32=1))[0, 0] == 257.0
    S = R.abs_product(R.desc(np.array([[1.0, -2.0]]), 1, 1, [R.group([[-3.0, 4.0]], 1, 0, 0)]))
    assert S[0, 0] == 11.0


# ------------------------------------------------------------------------------------------ host-only exports
def _lib():
    import _vc
    try:
        return _vc, _vc.lib()
    except _vc.VCError as e:                                 # pragma: no cover - the library is built by build()
        pytest.fail(str(e))


def host_desc(s, x_ptr=0x1000, bt_ptr=0x2000, c_ptr=0x3000):
    """GemmDesc of case s with made-up pointers: for the exports that only read the descriptor."""
    import _vc
    d = _vc.GemmDesc()
    d.dtype, d.mode, d.d_X, d.M, d.T, d.Cin, d.ldx, d.N, d.n_groups = s.dtype, s.mode, x_ptr, s.M, s.T, s.Cin, s.ldx, s.N, len(s.taps)
    for g, t in enumerate(s.taps):
        d.groups[g].d_Bt, d.groups[g].K, d.groups[g].taps, d.groups[g].pad_l, d.groups[g].c_off = bt_ptr, t * s.Cin, t, s.pad_l[g], s.c_off[g]
    d.pro_relu, d.pro_pool, d.act, d.ldr, d.d_C, d.ldc, d.out_f32 = s.pro_relu, s.pro_pool, s.act, s.ldr, c_ptr, s.ldc, s.out_f32
    if s.ldr:
        d.d_R = 0x4000
    if s.pro_affine:
        d.d_pro_scale = d.d_pro_shift = 0x5000
    d.drop_keep, d.sum_groups, d.epi_pool = s.drop_keep, s.sum_groups, s.epi_pool
    return d


def test_workspace_bytes_on_hand_made_descriptors():
    _vc, lib = _lib()
    ws = lambda s: lib.vc_conv_gemm_workspace_bytes(C.byref(host_desc(s)))
    assert lib.vc_conv_gemm_workspace_bytes(None) == 0
    for s in EXACT_CASES:
        want = 0
        if s.form == 'proj256' and s.Cin // 64 >= 8 and 2 * ((s.M + 255) // 256) <= 256:
            ntm = (s.M + 255) // 256
            want = ((ntm * 8 + 255) & ~255) + ntm * 262144      # tickets, then one 256 x 256 float32 tile per row tile
        assert ws(s) == want, (s.name, ws(s), want)
    big = case('w', 'proj256', BF16, 256 * 129, 256, 2048, 256, (2,), ldc=256, ldx=2048)   # 129 row tiles: two halves no longer fit one round
    assert expected_form(big) == 'proj256' and ws(big) == 0
    split = case('w', 'proj256', BF16, 1024, 256, 2048, 256, (2,), ldc=256, ldx=2048)
    assert ws(split) > 0
    try:
        _vc.set_option('proj256_split', 0)
        assert ws(split) == 0
        _vc.set_option('proj256_split', -1)
        _vc.set_option('proj256', 0)
        assert ws(split) == 0
    finally:
        _vc.set_option('proj256_split', -1)
        _vc.set_option('proj256', -1)
    for k, v in (('out_f32', 1), ('ldr', 256), ('pro_pool', 2), ('N', 128), ('M', 768), ('dtype', F32), ('sum_groups', 1)):
        t = case('w', 'x', BF16, 1024, 256, 2048, 256, (2,), ldc=256, ldx=2048)
        setattr(t, k, v)
        assert ws(t) == 0, k


def test_epi_pool_supported_on_hand_made_descriptors():
    _vc, lib = _lib()
    sup = lambda s: lib.vc_conv_gemm_epi_pool_supported(C.byref(host_desc(s)))
    assert lib.vc_conv_gemm_epi_pool_supported(None) == 0
    for s in EXACT_CASES:
        want = 1 if (s.form == 'bank256' and s.act == ACT_RELU) else 0
        assert sup(s) == want, (s.name, sup(s), want)
    base = dict(taps=(1, 2, 3, 4), pad_l=(0, 0, 1, 1), act=ACT_RELU, epi_pool=1, ldc=512, ldx=64)
    assert sup(case('p', 'bank256', BF16, 256, 64, 64, 128, **base)) == 1
    for k, v in (('act', ACT_NONE), ('M', 192), ('dtype', F32), ('N', 64), ('Cin', 32), ('out_f32', 1), ('ldr', 128), ('pro_pool', 1),
                 ('taps', (1, 2, 3, 5)), ('pad_l', (0, 0, 1, 2)), ('c_off', (0, 128, 256, 388)), ('ldc', 516), ('drop_keep', 0.5),
                 ('T', 7)):
        t = case('p', 'bank256', BF16, 256, 64, 64, 128, **base)
        setattr(t, k, v)
        if k == 'taps':
            t.taps = v
        assert sup(t) == 0, k
    odd = dict(base, taps=(1, 2, 3), pad_l=(0, 0, 1))
    assert sup(case('p', 'bank256', BF16, 256, 64, 64, 128, **odd)) == 0
    try:
        _vc.set_option('bank256', 0)
        assert sup(case('p', 'bank256', BF16, 256, 64, 64, 128, **base)) == 0
    finally:
        _vc.set_option('bank256', -1)
