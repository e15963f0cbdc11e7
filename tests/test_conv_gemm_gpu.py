"""vc_conv_gemm alone, through _vc.lib(), against the float64 definition of its descriptor (tests/conv_gemm_ref.py), over
every kernel form launch() of csrc/vc_gemm.hip can select:

    form         | condition in launch() (first match wins)
    -------------+--------------------------------------------------------------------------------------------------
    conv_kernel  | sum_groups != 0 (needs plain mode, Cin % slab == 0, M >= 128, taps <= 32; slab = 32 f32 / 64 bf16)
    proj256      | bf16, one group, N == 256, Cin % 64 == 0, M >= 1024, 2 <= taps <= 32, K >= 4096, no prologue / residual /
                 | out_f32 / dropout / epi_pool, act none | relu, C 16-byte aligned, ldx, ldc, c_off % 8 == 0, option proj256 != 0
                 | (K split in two given a 256-byte aligned workspace of vc_conv_gemm_workspace_bytes(), option proj256_split != 0)
    vc_conv256   | bf16, one group, N % 128 == 0, Cin % 64 == 0, M >= 128, taps <= 7, K >= 384 (option conv256_min_k), no affine /
                 | relu prologue, pro_pool != 1, no out_f32 / dropout, the same alignments, R 8-byte aligned and ldr % 4 == 0
    vc_bank256   | taps > 1 somewhere, all taps <= 32, Cin % slab == 0, M >= 128, plain mode; bf16, an even number of groups of
                 | N == 128 in pairs (taps, taps + 1) with a common pad_l, Cin % 64 == 0, M >= 256, no prologue / residual /
                 | out_f32 / dropout, act none | relu, the same alignments, option bank256 != 0
    conv_kernel  | the same first line without the bank conditions; PRO 2 with an affine or relu prologue, PRO 1 with pro_pool
    gemm_kernel  | everything else: MI = 1 below 512 blocks of 128 rows, MI = 2 from 512; highway mode; PRO as above

tests/conv_gemm_cases.py holds the table of exact cases and restates these conditions (expected_form);
tests/test_conv_gemm_cpu.py checks that every row lands on its form and stays exactly representable.  Nothing on the
device tells which form ran: the forms are told apart by that restatement alone.  Output buffers start as NaN; X, C and R live in wider allocations whose padding columns
hold NaN.  Lines starting with 'MEASURED' carry the device's errors next to their bounds (profiles/conv_gemm/README.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_gemm_ref as R
from conv_gemm_ref import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, BF16, F32, HIGHWAY
from conv_gemm_cases import (DROP_C_OFF, DROPOUT_CASES, ISOLATION_CASES, ORDER_CASES, ZERO_CASES, case, cases_of, expected_form,
                             make_exact, make_order, make_zeros, start_contents)

pytestmark = pytest.mark.gpu

TDT = {F32: torch.float32, BF16: torch.bfloat16}
EPS32, EPS16 = 2.0 ** -24, 2.0 ** -8
# largest |device - float64| of act_fn's sigmoid (__expf) and tanh (tanhf) over [-20, 20], measured by
# test_sigmoid_and_tanh_alone on an MI355X (8.78e-8 and 6.24e-8, profiles/conv_gemm/README.md); the test holds each to
# 4 x its value
SIGMOID_MAX, TANH_MAX = 8.8e-8, 6.3e-8


@pytest.fixture(autouse=True)
def _default_kernel_options():
    import _vc
    yield
    for n in ('bank256', 'conv256', 'proj256', 'proj256_split'):
        _vc.set_option(n, -1)


def _poison():
    from conftest import poison_gpu_state
    poison_gpu_state()


def _padded(a, ld, dtype):
    """[M, C] float64 -> device [M, ld] of dtype with NaN in the padding columns."""
    a = np.asarray(a, dtype=np.float64)
    out = torch.full((a.shape[0], ld), float('nan'), dtype=torch.float64)
    out[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a))
    return out.to(dtype).cuda()


def _vec(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).to(torch.float32).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


class Launch:
    """Device buffers and the vc_gemm_desc of a reference descriptor `d`."""

    def __init__(self, d, ldx, ldr=0, ws=None):
        import _vc
        self.d, self.ldr = d, ldr
        dt = TDT[d.dtype]
        self.odt = torch.float32 if (d.out_f32 or d.dtype == F32) else torch.bfloat16
        self.X = _padded(d.X, ldx, dt)
        self.W = [torch.from_numpy(np.ascontiguousarray(g.W)).to(dt).cuda() for g in d.groups]
        self.vecs = [_vec(v) for v in (d.pro_scale, d.pro_shift, d.epi_scale, d.epi_shift)]
        self.R = None if d.R is None else _padded(d.R, ldr or d.N, dt)
        g = _vc.GemmDesc()
        g.dtype, g.mode, g.d_X, g.M, g.T, g.Cin, g.ldx, g.N, g.n_groups = d.dtype, d.mode, _p(self.X), d.M, d.T, d.Cin, ldx, d.N, len(d.groups)
        for i, gr in enumerate(d.groups):
            g.groups[i].d_Bt, g.groups[i].K, g.groups[i].taps = _p(self.W[i]), gr.taps * d.Cin, gr.taps
            g.groups[i].pad_l, g.groups[i].c_off = gr.pad_l, gr.c_off
        g.d_pro_scale, g.d_pro_shift, g.d_epi_scale, g.d_epi_shift = (_p(v) for v in self.vecs)
        g.pro_relu, g.pro_pool, g.act, g.d_R, g.ldr, g.ldc, g.out_f32 = d.pro_relu, d.pro_pool, d.act, _p(self.R), ldr or d.N, d.ldc, d.out_f32
        g.drop_keep, g.drop_seed, g.sum_groups, g.epi_pool = d.drop_keep, d.drop_seed, d.sum_groups, d.epi_pool
        self.desc = g
        self.wsbuf = None
        if ws is not None:
            need = _vc.lib().vc_conv_gemm_workspace_bytes(C.byref(g))
            assert need > 0, 'the case expects a launch that can split K'
            if ws != 'none':
                self.wsbuf = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device='cuda')     # contents need not be initialised
                base = (self.wsbuf.data_ptr() + 255) & ~255
                g.d_workspace = base + (128 if ws == 'misaligned' else 0)
                g.workspace_bytes = need - 256 if ws == 'small' else need

    def run(self, C0=None, expect_error=None):
        """One launch into a fresh NaN-filled C (or C0); returns the device tensor [M, ldc]."""
        import _vc
        d = self.d
        if C0 is None:
            Cd = torch.full((d.M, d.ldc), float('nan'), dtype=self.odt, device='cuda')
        else:
            Cd = torch.from_numpy(np.ascontiguousarray(C0)).to(self.odt).cuda()
        self.desc.d_C = Cd.data_ptr()
        rc = _vc.lib().vc_conv_gemm(C.byref(self.desc), _vc.current_stream())
        if expect_error is None:
            _vc.check(rc)
        else:
            assert rc != 0
            with pytest.raises(_vc.VCError, match=expect_error):
                _vc.check(rc)
        torch.cuda.synchronize()
        return Cd


def _host(Cd):
    return Cd.detach().cpu().to(torch.float64).numpy()


def _bits(Cd):
    return Cd.view(torch.int32 if Cd.dtype == torch.float32 else torch.int16)


def _same_bits(c1, c2, what, nan_payload=True):
    """Two launches of one descriptor: identical raw bits.  nan_payload=False (poisoned inputs): NaN in the same places,
    identical bits everywhere else -- which NaN comes out of an operation on two NaNs is not specified."""
    if nan_payload:
        assert torch.equal(_bits(c1), _bits(c2)), what + ': two runs differ'
    else:
        n1, n2 = torch.isnan(c1), torch.isnan(c2)
        assert torch.equal(n1, n2), what + ': two runs have NaN in different places'
        assert torch.equal(_bits(c1)[~n1], _bits(c2)[~n2]), what + ': two runs differ'


def _run_twice(L, what, C0=None, nan_payload=True):
    c1 = L.run(C0)
    _same_bits(c1, L.run(C0), what, nan_payload)
    return c1


def _same(got, ref, what, rows=None):
    """Equal values in every element, NaN exactly where the reference has NaN (signed zeros compare equal)."""
    if rows is not None:
        got, ref = got[rows], ref[rows]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref, equal_nan=True):
        bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
        m, n = bad[0]
        raise AssertionError('%s: %d of %d elements differ, first at [%d, %d]: device %r, reference %r'
                             % (what, len(bad), got.size, m, n, got[m, n], ref[m, n]))


def _run_exact(s, d=None):
    import _vc
    d = make_exact(s) if d is None else d
    C0 = start_contents(s, d)
    ref = R.conv_gemm(d, C0=C0)
    L = Launch(d, s.ldx, s.ldr, s.ws)
    c1 = L.run(C0)
    _same(_host(c1), ref, s.name)
    c2 = L.run(C0)
    # (sum_groups > 1 is documented as order-dependent; on the integer grid every order gives the same sum)
    _same_bits(c1, c2, s.name)
    for opt in s.toggle:
        with _vc.options(**{opt: 0}):
            c3 = L.run(C0)
        assert torch.equal(_bits(c1), _bits(c3)), '%s: differs with option %s = 0' % (s.name, opt)
    return L, c1, ref


# ------------------------------------------------------------------------------------------ a. exact cases
FORM_DTYPES = [(f, dt) for f in ('gemm_mi1', 'gemm_mi2', 'highway_mi1', 'conv_kernel') for dt in (F32, BF16)] + \
              [(f, BF16) for f in ('conv256', 'bank256', 'proj256')]


@pytest.mark.parametrize('form,dtype', FORM_DTYPES, ids=['%s-%s' % (f, ('f32', 'bf16')[dt]) for f, dt in FORM_DTYPES])
def test_exact_cases_equal_the_reference_bit_for_bit(form, dtype):
    """Integer-grid operands (tests/test_conv_gemm_cpu.py proves every partial sum < 2^24 and every bf16-stored result an
    integer <= 256): the device result must EQUAL the float64 reference, element for element, padding columns still NaN,
    twice with identical bits, and identically with the form's option switched off."""
    rows = cases_of(form, dtype)
    assert rows
    _poison()
    failed = []
    for s in rows:
        assert expected_form(s) == form
        try:
            _run_exact(s)
        except AssertionError as e:                        # every case runs: the first failure does not hide the rest
            failed.append(str(e))
    assert not failed, '%d of %d cases fail:\n%s' % (len(failed), len(rows), '\n'.join(failed))


# ------------------------------------------------------------------------------------------ b. isolation of windows
ISOLATION = ISOLATION_CASES


@pytest.mark.parametrize('s', ISOLATION, ids=[s.name for s in ISOLATION])
def test_a_poisoned_window_does_not_reach_its_neighbours(s):
    """Three windows; the middle one is all NaN, then finite with +inf in its first and last frames.  SAME-padding zeros
    are selects, so the outer windows must equal the reference exactly (taps > 1, operand pool on, pooled epilogue),
    and two launches must give identical bits."""
    assert expected_form(s) == s.form
    T = s.T
    outer = np.r_[0:T, 2 * T:3 * T]
    _poison()
    for poison in ('nan', 'inf'):
        d = make_exact(s)
        if poison == 'nan':
            d.X[T:2 * T] = np.nan
        else:
            d.X[T] = np.inf
            d.X[2 * T - 1] = np.inf
        ref = R.conv_gemm(d)
        assert np.isfinite(ref[outer][:, :R.out_width(d)]).all()
        what = '%s (%s)' % (s.name, poison)
        got = _host(_run_twice(Launch(d, s.ldx, s.ldr, s.ws), what, nan_payload=False))
        _same(got, ref, what, rows=outer)


# ------------------------------------------------------------------------------------------ c. prologue order
@pytest.mark.parametrize('s', ORDER_CASES, ids=[s.name for s in ORDER_CASES])
def test_padding_stays_zero_behind_a_shifting_prologue(s):
    """X = 0, pro_scale = 1, pro_shift = 1, no ReLU, all-ones weights: every REAL frame contributes Cin, every padding
    frame must contribute 0 -- frames next to a window edge see fewer taps, and the result says how many."""
    assert expected_form(s) == s.form
    d = make_order(s)
    taps, pad_l = s.taps[0], s.pad_l[0]
    t = np.arange(s.M) % s.T
    real = np.minimum(s.T - 1, t + taps - 1 - pad_l) - np.maximum(0, t - pad_l) + 1
    ref = R.conv_gemm(d)
    assert np.array_equal(ref[:, :3], np.repeat((s.Cin * real)[:, None], 3, 1).astype(np.float64))
    _poison()
    _same(_host(_run_twice(Launch(d, s.ldx), s.name)), ref, s.name)


# ------------------------------------------------------------------------------------------ d. signed zeros
@pytest.mark.parametrize('s', ZERO_CASES, ids=[s.name for s in ZERO_CASES])
def test_non_negative_pool_orders_signed_zeros_as_values(s):
    """-0.0 and +0.0 next to positive values through the integer-ordered maximum: max(-0.0, 1.0) is 1.0, max(-0.0, +0.0)
    is a zero.  Results are compared as VALUES (the two zeros are the same value)."""
    assert expected_form(s) == s.form
    d = make_zeros(s)
    ref = R.conv_gemm(d)
    assert np.abs(ref[:, :s.N]).max() <= 256
    L = Launch(d, s.ldx)
    assert bool((L.X[:, :s.Cin] == 0).any()) and bool(torch.signbit(L.X[:, :s.Cin].float()).any())
    _poison()
    _same(_host(_run_twice(L, s.name)), ref, s.name)


# ------------------------------------------------------------------------------------------ e. dropout
@pytest.mark.parametrize('s', DROPOUT_CASES, ids=[s.name for s in DROPOUT_CASES])
def test_dropout_mask_is_the_host_mask(s):
    """The kept set equals tests/conv_gemm_ref.py's drop_mask of index m * ldc + c_off + n (ldc > N, c_off > 0); kept
    values are v / keep, dropped ones exactly 0 before the residual is added."""
    M, N, keep, seed, c_off = s.M, s.N, s.drop_keep, s.drop_seed, DROP_C_OFF
    assert expected_form(s) == s.form and s.ldc > c_off + N
    _poison()
    mask = R.drop_mask(M, s.ldc, N, seed, keep, c_off)
    assert keep < 1.0 or mask.all()
    assert keep == 1.0 or abs(mask.mean() - keep) < 0.05
    # ReLU on the integer grid with a residual: exact, v / keep included (one correctly rounded float32 division)
    d = make_exact(s)
    L, c1, ref = _run_exact(s, d)
    got = _host(c1)[:, c_off:c_off + N]
    assert np.array_equal(got[mask == 0], d.R[mask == 0])
    # tanh of half-integers (never 0), no residual: the kept set is the set of non-zero outputs
    d.epi_shift = np.full(c_off + N, 0.5)
    d.epi_scale = None
    d.act, d.R = ACT_TANH, None
    ref = R.conv_gemm(d, round_out=False)[:, c_off:c_off + N]
    got = _host(_run_twice(Launch(d, s.ldx), s.name + ' tanh'))
    assert np.isnan(got[:, :c_off]).all() and np.isnan(got[:, c_off + N:]).all()
    got = got[:, c_off:c_off + N]
    assert np.array_equal(got != 0.0, mask != 0.0)
    assert np.abs(got - ref).max() <= 4 * TANH_MAX / keep + 2 * EPS32 / keep


# ------------------------------------------------------------------------------------------ f. real-valued cases
def _glorot(rng, n, k):
    lim = np.sqrt(6.0 / (n + k))
    return rng.uniform(-lim, lim, (n, k))


REAL = [case('real_gemm_mi1', 'gemm_mi1', F32, 129, 43, 40, 129, (3,), act=ACT_TANH, ldr=132),
        case('real_gemm_mi1', 'gemm_mi1', BF16, 129, 43, 40, 129, (3,), act=ACT_SIGMOID, pro_affine=1, pro_relu=1, pro_pool=1),
        case('real_gemm_mi2', 'gemm_mi2', F32, 65536, 64, 8, 100, act=ACT_RELU),
        case('real_gemm_mi2', 'gemm_mi2', BF16, 65536, 64, 8, 100, act=ACT_RELU, out_f32=1),
        case('real_highway', 'highway_mi1', F32, 129, 129, 72, 192, mode=HIGHWAY, ldc=80, epi_scale=0),
        case('real_highway', 'highway_mi1', BF16, 129, 129, 72, 192, mode=HIGHWAY, ldc=80, epi_scale=0),
        case('real_conv_kernel', 'conv_kernel', F32, 255, 85, 64, 129, (7,), pro_affine=1, pro_relu=1, pro_pool=1, act=ACT_RELU, ldr=132),
        case('real_conv_kernel', 'conv_kernel', BF16, 255, 85, 64, 129, (7,), pro_affine=1, pro_pool=1, ldr=132),
        case('real_sum_groups', 'conv_kernel', F32, 256, 64, 32, 129, (1, 2, 3, 4), sum_groups=1, ldr=132),
        case('real_sum_groups_S2', 'conv_kernel', BF16, 256, 64, 64, 129, (1, 2, 3, 4), sum_groups=2, out_f32=1, epi_scale=0, epi_shift=0),
        case('real_conv256', 'conv256', BF16, 2048, 256, 512, 128, (3,), pro_pool=2, act=ACT_NONE, ldr=132, ldc=136, ldx=520),
        case('real_bank256', 'bank256', BF16, 511, 73, 128, 128, tuple(range(1, 9)), pad_l=tuple((k - 1) // 2 if k % 2 else (k - 2) // 2 for k in range(1, 9)),
             act=ACT_RELU, epi_pool=1, ldc=1032, ldx=136),
        case('real_proj256_split', 'proj256', BF16, 1025, 205, 2048, 256, (2,), ldc=264, ldx=2056, ws='full', act=ACT_RELU),
        case('real_proj256', 'proj256', BF16, 1025, 205, 128, 256, (32,), ldc=264, ldx=136)]


def _make_real(s):
    rng = np.random.RandomState(11)
    q = R.bf16_round if s.dtype == BF16 else R.f32_round
    xw = (max(s.c_off) + s.Cin) if s.sum_groups else s.Cin
    X = rng.standard_normal((s.M, xw))
    if s.pro_pool == 2 and not s.pro_relu:
        X = np.abs(X)
    X = q(X)
    f = R.f32_round
    pro_scale = f(rng.uniform(0.5, 1.5, s.Cin)) if s.pro_affine else None
    pro_shift = f(rng.standard_normal(s.Cin) * 0.5) if s.pro_affine else None
    if s.mode == HIGHWAY:
        H = s.Cin
        Bt, sh = R.highway_pack(_glorot(rng, H, H), rng.standard_normal(H) * 0.5, _glorot(rng, H, H), rng.standard_normal(H) * 0.5)
        return R.desc(X, s.T, s.N, [R.group(q(Bt), 1, 0, 0)], dtype=s.dtype, mode=HIGHWAY, epi_shift=f(sh), ldc=s.ldc, out_f32=s.out_f32)
    groups = [R.group(q(_glorot(rng, s.N, t * s.Cin)), t, p, c) for t, p, c in zip(s.taps, s.pad_l, s.c_off)]
    width = s.N if s.sum_groups else max(s.c_off) + s.N
    return R.desc(X, s.T, s.N, groups, dtype=s.dtype, Cin=s.Cin, pro_scale=pro_scale, pro_shift=pro_shift, pro_relu=s.pro_relu,
                  pro_pool=s.pro_pool, epi_scale=f(rng.uniform(0.5, 1.5, width)) if s.epi_scale else None,
                  epi_shift=f(rng.standard_normal(width) * 0.5) if s.epi_shift else None, act=s.act,
                  R=q(rng.standard_normal((s.M, s.N))) if s.ldr else None, ldc=s.ldc, out_f32=s.out_f32, sum_groups=s.sum_groups,
                  epi_pool=s.epi_pool)


@pytest.mark.parametrize('s', REAL, ids=['%s-%s' % (s.name, ('f32', 'bf16')[s.dtype]) for s in REAL])
def test_real_valued_cases_within_the_float32_accumulation_bound(s):
    """Standard-normal X, Glorot weights, operands pre-rounded to the storage type.  Per element, with S = sum |A| |B| from
    the reference and K the contraction length:
        |pre - ref_pre| <= 2 (K + 4) 2^-24 (|s| S + |b|)        float32 accumulation in any order; the 2 covers truncation
                         + 2^-8 |s| S                            bf16 affine prologue: one re-rounding of each operand
    pushed through the activation (Lipschitz 1 for ReLU / tanh, 1/4 for sigmoid; 4 x the measured error of the device's
    sigmoid / tanh themselves), + 3 * 2^-24 (|v| + |R[m, n]|) for the activation's, the residual add's and the store's
    float32 roundings (R: the residual, or what C held where sum_groups > 1 adds to it), + 2^-8 |v| for bf16 storage.
    The first two lines and the storage term are the issue's; the others are added because its formula stops at the
    pre-activation.  Two launches must give identical bits, except where sum_groups > 1 makes the order free.  Highway: the two pre-activation bounds through relu(h) t + x (1 - t) with
    |dt| <= |dpre_t| / 4 + 2^-21 (v_exp_f32 / v_rcp_f32 at 1 ulp each, and the sum 1 + e)."""
    assert expected_form(s) == s.form
    d = _make_real(s)
    K = sum(g.taps for g in d.groups) * d.Cin if d.sum_groups else max(g.taps for g in d.groups) * d.Cin
    stored16 = d.dtype == BF16 and not d.out_f32
    parts = {}
    C0 = None
    if d.sum_groups > 1:
        C0 = np.full((d.M, d.ldc), np.nan)
        C0[:, :d.N] = R.f32_round(np.random.RandomState(12).standard_normal((d.M, d.N)))
    ref = R.conv_gemm(d, C0=C0, round_out=False, parts=parts)
    _poison()
    L = Launch(d, s.ldx, s.ldr, s.ws)
    got = _host(L.run(C0) if d.sum_groups > 1 else _run_twice(L, s.name, C0))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), s.name + ': written set differs'
    acc_eps = 2.0 * (K + 4) * EPS32
    if d.mode == HIGHWAY:
        H = d.Cin
        b = np.abs(np.asarray(d.epi_shift))
        h = np.arange(H)
        col = 64 * (h // 32) + h % 32
        e_h = acc_eps * (parts['S_h'] + b[col][None, :])
        e_t = acc_eps * (parts['S_t'] + b[col + 32][None, :]) / 4 + 2.0 ** -21
        hv, x = np.maximum(parts['hpre'], 0.0), d.X[:, :H]
        v = ref[:, :H]
        bound = e_h + np.abs(hv - x) * e_t + e_h * e_t + 3 * EPS32 * (np.abs(v) + np.abs(x))
        w = np.zeros_like(ref, dtype=bool)
        w[:, :H] = True
        bound_full = np.zeros_like(ref)
        bound_full[:, :H] = bound
        bound = bound_full
    else:
        w = ~np.isnan(ref)
        S = parts['S']
        sc = np.zeros(d.ldc)
        sh = np.zeros(d.ldc)
        for g in ([R.group(np.zeros((1, 1)), 1, 0, 0)] if d.sum_groups else d.groups):
            sc[g.c_off:g.c_off + d.N] = np.abs(R._coef(d.epi_scale, g.c_off, d.N, 1.0))
            sh[g.c_off:g.c_off + d.N] = np.abs(R._coef(d.epi_shift, g.c_off, d.N, 0.0))
        bound = acc_eps * (sc[None, :] * S + sh[None, :])
        if d.dtype == BF16 and d.pro_scale is not None:
            bound = bound + EPS16 * sc[None, :] * S
        bound = bound * (0.25 if d.act == ACT_SIGMOID else 1.0) + {ACT_SIGMOID: 4 * SIGMOID_MAX, ACT_TANH: 4 * TANH_MAX}.get(d.act, 0.0)
        if d.epi_pool:
            bound = R.pool_same(np.where(w, bound, 0.0), d.T)              # |max(a, b) - max(a', b')| <= max of the two errors
        r = np.zeros_like(ref)
        if d.R is not None:
            for g in ([R.group(np.zeros((1, 1)), 1, 0, 0)] if d.sum_groups else d.groups):
                r[:, g.c_off:g.c_off + d.N] = np.abs(np.asarray(d.R))
        elif C0 is not None:
            r = np.nan_to_num(np.abs(C0))
        bound = bound + 3 * EPS32 * (np.abs(ref) + r)
    if stored16:
        bound = bound + EPS16 * np.abs(ref)
    ratio = (np.abs(got - ref)[w] / bound[w]).max()
    print('MEASURED %s %s K=%d err=%.3e err/bound=%.3f' % (s.name, ('f32', 'bf16')[s.dtype], K, np.abs(got - ref)[w].max(), ratio))
    assert ratio <= 1.0, (s.name, ratio)


# ------------------------------------------------------------------------------------------ g. sigmoid and tanh alone
def _act_inputs():
    one = np.float32(1.0)
    tiny = [np.nextafter(np.float32(0), one) * k for k in (1, 2, 3)] + [np.float32(2.0 ** -126) * k for k in (1, 2, 3)]
    x = np.concatenate([np.linspace(-20, 20, 16001), np.array(tiny, dtype=np.float64), -np.array(tiny, dtype=np.float64), [0.0, -0.0],
                        np.float64(2.0) ** np.arange(-30, 5), -(np.float64(2.0) ** np.arange(-30, 5))])
    x = R.f32_round(x)
    n = (len(x) + 7) // 8 * 8
    return np.concatenate([x, np.zeros(n - len(x))]).reshape(-1, 8)


@pytest.mark.parametrize('act,name,recorded', [(ACT_SIGMOID, 'sigmoid', SIGMOID_MAX), (ACT_TANH, 'tanh', TANH_MAX)])
def test_sigmoid_and_tanh_alone(act, name, recorded):
    """act_fn uses __expf / tanhf, whose error has no derivation: identity weights make acc = x exactly, the outputs are
    compared with float64 over [-20, 20], 0 and a few ULPs either side of it.  Holds each to 4 x its recorded maximum, and
    fails outright if that exceeds 2e-5 (the float32 tolerance of tests/test_blocks_gpu.py)."""
    assert 4 * recorded <= 2e-5
    X = _act_inputs()
    d = R.desc(X, 1, 8, [R.group(np.eye(8), 1, 0, 0)], act=act, ldc=8)
    ref = R.conv_gemm(d, round_out=False)
    _poison()
    got = _host(_run_twice(Launch(d, 8), 'act_fn ' + name))
    err = np.abs(got - ref).max()
    print('MEASURED act_fn %s max|err|=%.3e over %d inputs (recorded %.1e)' % (name, err, X.size, recorded))
    assert err <= 4 * recorded, (name, err)


# ------------------------------------------------------------------------------------------ h. rejections
def _valid(dtype=F32, **kw):
    slab = 32 if dtype == F32 else 64
    s = case('rej', 'x', dtype, kw.pop('M', 128), kw.pop('T', 32), kw.pop('Cin', slab), kw.pop('N', 16), kw.pop('taps', (3,)), **kw)
    return s, make_exact(s)


def _set(**fields):
    def f(L):
        for k, v in fields.items():
            setattr(L.desc, k, v)
    return f


def _grp(g, **fields):
    def f(L):
        for k, v in fields.items():
            setattr(L.desc.groups[g], k, v)
    return f


def _ptr_off(field, nbytes, g=None):
    def f(L):
        tgt = L.desc if g is None else L.desc.groups[g]
        setattr(tgt, field, getattr(tgt, field) + nbytes)
    return f


HW = dict(mode=HIGHWAY, M=65, T=65, Cin=40, N=128, taps=(1,), ldc=48, epi_scale=0)
SUMS = dict(taps=(1, 2, 3), sum_groups=2, out_f32=1, epi_scale=0, epi_shift=0)
REJECTIONS = [
    ('M_not_multiple_of_T', {}, _set(T=33), r'M \(128\) must be a multiple of T'),
    ('K_not_taps_times_Cin', {}, _grp(0, K=3 * 32 + 4), r'K \(100\) != taps'),
    ('pad_l_negative', {}, _grp(0, pad_l=-1), 'bad pad_l'),
    ('pad_l_equals_taps', {}, _grp(0, pad_l=3), 'bad pad_l'),
    ('Cin_not_multiple_of_vec', {}, _set(Cin=30), r'Cin \(30\) and ldx \(36\) must be multiples of 4'),
    ('ldx_not_multiple_of_vec', {}, _set(ldx=38), r'Cin \(32\) and ldx \(38\) must be multiples of 4'),
    ('ldx_below_Cin', {}, _set(ldx=28), 'with ldx >= Cin'),
    ('X_misaligned', {}, _ptr_off('d_X', 4), 'X must be 16-byte aligned'),
    ('Bt_misaligned', {}, _ptr_off('d_Bt', 8, g=0), 'Bt NULL or misaligned'),
    ('pro_scale_without_shift', dict(pro_affine=1), _set(d_pro_shift=None), 'pro_scale and pro_shift go together'),
    ('pro_shift_without_scale', dict(pro_affine=1), _set(d_pro_scale=None), 'pro_scale and pro_shift go together'),
    ('highway_with_residual', HW, lambda L: _set(d_R=L.X.data_ptr(), ldr=48)(L), 'highway mode'),
    ('highway_two_taps', HW, _grp(0, taps=2, K=80, pad_l=0), 'highway mode'),
    ('highway_N_not_64_multiple', HW, _set(N=96), 'highway mode'),
    ('highway_N_below_2H', dict(HW, Cin=72, N=192, ldc=80), _set(N=128), 'highway mode'),
    ('sum_groups_S_with_shift', SUMS, lambda L: _set(d_epi_shift=L.X.data_ptr())(L), 'sum_groups > 1'),
    ('sum_groups_S_with_activation', SUMS, _set(act=ACT_RELU), 'sum_groups > 1'),
    ('sum_groups_S_too_many_splits', SUMS, _set(sum_groups=3), 'sum_groups > 1'),
    ('sum_groups_S_bf16_output', dict(SUMS, dtype=BF16), _set(out_f32=0), 'sum_groups > 1'),
    ('sum_groups_small_M', dict(SUMS, sum_groups=1, M=96), None, 'sum_groups needs'),
    ('sum_groups_channels_outside_row', dict(SUMS, sum_groups=1), _grp(2, c_off=96), r'sum_groups\): input channels'),
    ('epi_pool_on_generic_kernel', dict(act=ACT_RELU), _set(epi_pool=1), 'epi_pool'),
    ('epi_pool_without_relu', dict(dtype=BF16, M=256, T=64, N=128, taps=(1, 2), pad_l=(0, 0), ldc=264, ldx=72), _set(epi_pool=1), 'epi_pool'),
    ('columns_past_ldc', {}, _set(ldc=15), 'columns exceed ldc'),
    ('c_off_pushes_columns_past_ldc', {}, _grp(0, c_off=6), 'columns exceed ldc'),
    ('drop_keep_above_one', {}, _set(drop_keep=1.5), 'drop_keep'),
    ('drop_keep_negative', {}, _set(drop_keep=-0.25), 'drop_keep'),
]


@pytest.mark.parametrize('name,kw,mutate,message', REJECTIONS, ids=[r[0] for r in REJECTIONS])
def test_invalid_descriptors_are_rejected_on_the_host(name, kw, mutate, message):
    """Every VC_REQUIRE of vc_conv_gemm and launch(): an error through _vc.check whose message names the field, and the
    NaN-filled C untouched (nothing is launched)."""
    _poison()
    kw = dict(kw)
    s, d = _valid(kw.pop('dtype', F32), **kw)
    L = Launch(d, s.ldx, s.ldr)
    C0 = start_contents(s, d)
    if mutate is not None:
        ok = L.run(C0)                                         # the unmutated descriptor is valid
        assert bool(torch.isfinite(ok[:, :1]).all())
        mutate(L)
    Cd = L.run(None, expect_error=message)
    assert bool(torch.isnan(Cd).all()), name + ': C was written'
