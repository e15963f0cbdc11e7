"""Every training kernel alone (csrc/vc_train.hip, vc_conv_wgrad of csrc/vc_gemm.hip), called through _vc.lib() and
compared with the float64 definitions of tests/train_kernels_ref.py at the shapes where the host code takes another
branch or a block / tile / window edge falls.  Output buffers are NaN-filled first: an element that was not written, or
one written where it must not be, both show.  Lines starting with 'MEASURED' carry the device's errors next to their
bounds (profiles/train_kernels/README.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_kernels_ref as R
from test_train_kernels_cpu import ROUTING_SHAPES, routing_inputs

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS32 = 2.0 ** -24              # one float32 rounding, relative
BIG_N = 8192 * 256 + 257        # past the 8,192-block cap of the grid-stride kernels


def _lib():
    import _vc
    return _vc.lib()


def _check(rc):
    import _vc
    _vc.check(rc)


def _st():
    import _vc
    return _vc.current_stream()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    a = a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return a.to(torch.float32).contiguous().cuda()


def nans(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().to(F64)


def padded(a, ld):
    """[M, C] -> device [M, ld] float32 with NaN in the padding columns."""
    a = torch.as_tensor(np.asarray(a)).to(torch.float32)
    out = torch.full((a.shape[0], ld), float('nan'), dtype=torch.float32)
    out[:, :a.shape[1]] = a
    return out.cuda()


def f32(a):
    """float64 tensor holding exactly the float32 values the device is given."""
    return torch.as_tensor(np.asarray(a)).to(torch.float32).to(F64)


def _within(got, want, bound, what=''):
    got, want, bound = (torch.as_tensor(a).to(F64) for a in (got, want, bound))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what + ': not written / not finite'
    over = (got - want).abs() - bound
    assert float(over.max()) <= 0.0, (what, float(over.max()), float((got - want).abs().max()))


def _rel_max(got, want):
    want = torch.as_tensor(want).to(F64)
    assert bool(torch.isfinite(got).all())
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-300))


# ------------------------------------------------------------------------------------------ batch statistics

BN_EPS, BN_DECAY = float(np.float32(1e-3)), float(np.float32(0.9))


@pytest.mark.parametrize('ratio', [0, 4, 32, 256])
@pytest.mark.parametrize('M,Cn,ld', [(1, 1, 1), (63, 33, 40), (64, 32, 32), (65, 257, 300), (640, 96, 96), (200, 520, 520)])
def test_bn_train_stats_offset_means(M, Cn, ld, ratio):
    """vc_bn_train_stats on columns whose mean is `ratio` standard deviations from zero (sigma 1.0 and 0.05), with and
    without moving statistics, NaN in the padding columns: mean, rstd, scale, shift and the moving values against float64.
    Bound: 8 x the error the float32 two-pass restatement (train_kernels_ref.bn_stats_f32) makes on the same input (the
    kernel adds 64-row blocks in another order), at least 1e-6; errors relative to train_kernels_ref.bn_stats_magnitude.
    Row counts: one block short by one row (63), exactly one (64), one row into the second (65), ten blocks (640), a
    ragged fourth (200); channel counts on both sides of the 256-thread block and the finalizer's 32-channel group.
    The sum(x^2) / M - mean^2 form this kernel had failed here at ratios 32 and 256 (rstd off by 1.5e-4 and 1e-2)."""
    lib = _lib()
    rng = np.random.RandomState(M + Cn + ratio)
    for sigma in (1.0, 0.05):
        sign = np.where(np.arange(Cn) % 2 == 0, 1.0, -1.0)
        X32 = ((rng.standard_normal((M, Cn)) + ratio * sign) * sigma).astype(np.float32)
        gamma, beta = rng.uniform(0.5, 1.5, Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32)
        mm0, mv0 = rng.standard_normal(Cn).astype(np.float32), rng.uniform(0.5, 2.0, Cn).astype(np.float32)
        Xd, gd, bd = padded(X32, ld), dev(gamma), dev(beta)
        for moving in (True, False):
            args = (f32(X32), f32(gamma), f32(beta), BN_EPS) + ((f32(mm0), f32(mv0), BN_DECAY) if moving else ())
            want, two_pass, mag = R.bn_stats(*args), R.bn_stats_f32(*args), R.bn_stats_magnitude(*args)
            out = {k: nans(Cn + 1) for k in ('scale', 'shift', 'mean', 'rstd')}
            mm, mv = (torch.cat([dev(mm0), nans(1)]), torch.cat([dev(mv0), nans(1)])) if moving else (None, None)
            nws = lib.vc_stats_workspace_floats(M, Cn)
            ws = nans(nws + 1)
            _check(lib.vc_bn_train_stats(p(Xd), M, Cn, ld, p(gd), p(bd), p(mm), p(mv), BN_DECAY, BN_EPS,
                                         p(out['scale']), p(out['shift']), p(out['mean']), p(out['rstd']), p(ws), _st()))
            if moving:
                out['moving_mean'], out['moving_var'] = mm, mv
            assert bool(torch.isnan(host(ws)[nws:]).all()), 'wrote past vc_stats_workspace_floats'
            for k, t in out.items():
                got = host(t)
                assert bool(torch.isnan(got[Cn:]).all()), k + ': wrote past C'
                err = float(((got[:Cn] - want[k]).abs() / mag[k]).max())
                tol = max(8.0 * float(((two_pass[k] - want[k]).abs() / mag[k]).max()), 1e-6)
                print('MEASURED bn_train_stats M=%d C=%d ratio=%d sigma=%g moving=%d %s err=%.2e bound=%.2e'
                      % (M, Cn, ratio, sigma, moving, k, err, tol))
                assert err <= tol, (k, sigma, moving, err, tol)


# ------------------------------------------------------------------------------------------ batch-norm backward / routing

def _bn_backward_dev(G, X, M, Cn, ld, T, gamma, st, mode):
    lib = _lib()
    dX, dgamma, dbeta = nans(M, ld), nans(Cn + 1), nans(Cn + 1)
    ws = nans(lib.vc_stats_workspace_floats(M, Cn))
    _check(lib.vc_bn_backward(p(G), p(X), M, Cn, ld, T, p(gamma), p(st['scale']), p(st['shift']), p(st['mean']),
                              p(st['rstd']), mode, p(dX), p(dgamma), p(dbeta), p(ws), _st()))
    dX, dgamma, dbeta = host(dX), host(dgamma), host(dbeta)
    assert bool(torch.isnan(dX[:, Cn:]).all()) and bool(torch.isnan(dgamma[Cn:]).all()) and bool(torch.isnan(dbeta[Cn:]).all())
    return dX[:, :Cn], dgamma[:Cn], dbeta[:Cn]


def _routing_dev(X, M, Cn, ld, T, scale, shift):
    bits = torch.full((M * Cn + 1,), 0xAA, dtype=torch.uint8, device='cuda')
    _check(_lib().vc_bn_post_routing(p(X), M, Cn, ld, T, p(scale), p(shift), p(bits), _st()))
    torch.cuda.synchronize()
    b = bits.cpu()
    assert int(b[-1]) == 0xAA
    return b[:-1].view(M, Cn)


@pytest.mark.parametrize('N,T,Cn,ld', ROUTING_SHAPES)
def test_bn_backward_and_routing_random_inputs(N, T, Cn, ld):
    """vc_bn_post_routing and vc_bn_backward (modes 0, 1, 2) on random floats, ld > C with NaN padding.  The 64-row blocks
    of the pass kernels end inside a window (T = 50, M = 400), on window edges (T = 64; T = 4 and 1 trivially) and past
    M (M = 50, 52 < 64; 100, 200, 320 ragged last blocks); C = 1, 33, 257 (one thread, a partial wave, a second block of
    256 channels).  The device's bits equal the float64 bits wherever no compared pair of activations is closer than
    1e-5 (at most 1 % excluded; tests/test_train_kernels_cpu.py holds the reference alone to that cap on these inputs);
    dX, dgamma, dbeta against float64 given the device's bits, 1e-4 of each tensor's maximum."""
    M = N * T
    X32, scale, shift = routing_inputs(M, Cn, ld, N + T + Cn)
    rng = np.random.RandomState(7 * N + T)
    Xv = f32(X32[:, :Cn])
    gamma = rng.uniform(0.5, 1.5, Cn).astype(np.float32)
    mean = rng.standard_normal(Cn).astype(np.float32) * 0.2
    rstd = (scale / gamma).astype(np.float32)                     # scale = gamma rstd, as vc_bn_train_stats leaves them
    G32 = np.full((M, ld), np.nan, np.float32)
    G32[:, :Cn] = rng.standard_normal((M, Cn))
    Xd, Gd = torch.from_numpy(X32).cuda(), torch.from_numpy(G32).cuda()
    st = dict(scale=dev(scale), shift=dev(shift), mean=dev(mean), rstd=dev(rstd))
    bits = _routing_dev(Xd, M, Cn, ld, T, st['scale'], st['shift'])
    want_bits = R.routing_bits(Xv, f32(scale), f32(shift), T)
    close = R.routing_close(Xv, f32(scale), f32(shift), T)
    assert float(close.to(F64).mean()) <= 0.01
    assert bool((bits == want_bits)[~close].all()), int((bits != want_bits)[~close].sum())
    for mode in (0, 1, 2):
        gd = dev(gamma)
        dX, dgamma, dbeta = _bn_backward_dev(Gd, Xd, M, Cn, ld, T, gd, st, mode)
        rX, rg, rb = R.bn_backward(f32(G32[:, :Cn]), Xv, T, f32(gamma), f32(mean), f32(rstd), mode, bits)
        errs = [_rel_max(a, b) for a, b in ((dX, rX), (dgamma, rg), (dbeta, rb))]
        print('MEASURED bn_backward N=%d T=%d C=%d mode=%d dX=%.2e dgamma=%.2e dbeta=%.2e bound=1e-4' % ((N, T, Cn, mode) + tuple(errs)))
        assert max(errs) < 1e-4, (mode, errs)


@pytest.mark.parametrize('N,T,Cn,ld', [(64, 1, 33, 40), (16, 4, 257, 260), (8, 50, 1, 3), (4, 64, 33, 64), (2, 64, 1, 1)])
def test_bn_backward_and_routing_tie_rule_on_integer_grid(N, T, Cn, ld):
    """Activations on the integer grid -2 .. 3 with scale = 1, shift = 0 (mean 0, rstd 1, gamma 1), integer gradients:
    every comparison is exact and ties are frequent (one pair in six).  The bits must EQUAL the float64 bits everywhere --
    own frame on >=, previous frame on strict >, nothing through a zero activation, a window's last frame never looks
    past it (train_kernels_ref.routing_bits; its tie rule is pinned on a hand-written column in the CPU file) -- and
    mode 2 of vc_bn_backward must take the same decisions: dbeta = sum d and dgamma = sum d x are sums of small integers,
    exact in float32, and must equal the reference exactly; dX = d - dbeta / M - x dgamma / M within four float32
    roundings of its largest term (1 / M is not a float32 number; a wrong decision moves d by a whole unit)."""
    M = N * T
    rng = np.random.RandomState(N + T + Cn)
    X = rng.randint(-2, 4, (M, Cn)).astype(np.float32)
    G = rng.randint(-3, 4, (M, Cn)).astype(np.float32)
    one, zero = np.ones(Cn, np.float32), np.zeros(Cn, np.float32)
    Xd, Gd = padded(X, ld), padded(G, ld)
    st = dict(scale=dev(one), shift=dev(zero), mean=dev(zero), rstd=dev(one))
    bits = _routing_dev(Xd, M, Cn, ld, T, st['scale'], st['shift'])
    want_bits = R.routing_bits(f32(X), f32(one), f32(zero), T)
    assert bool((bits == want_bits).all()), int((bits != want_bits).sum())
    for mode in (1, 2):
        dX, dgamma, dbeta = _bn_backward_dev(Gd, Xd, M, Cn, ld, T, st['scale'], st, mode)
        rX, rg, rb = R.bn_backward(f32(G), f32(X), T, f32(one), f32(zero), f32(one), mode, want_bits)
        assert bool((dbeta == rb).all()) and bool((dgamma == rg).all()), mode
        big = 3.0 + rb.abs() / M + 3.0 * rg.abs() / M
        _within(dX, rX, (4 * EPS32 * big).expand_as(rX), 'dX mode %d' % mode)


# ------------------------------------------------------------------------------------------ transpose_pad

@pytest.mark.parametrize('Cn', [1, 31, 33, 80])
@pytest.mark.parametrize('M,T', [(31, 31), (32, 4), (33, 11), (100, 25)])
def test_transpose_pad_prologue_and_margins(M, T, Cn):
    """vc_transpose_pad around its 32 x 32 tile (M, C one below / at / one above it, several tiles), row_shift -T (every
    frame leaves its window), -1, 0, 1, T - 1, relu / pool / affine each on and off, pad 0 / 32 / 37 with ldt > M + 2 pad,
    slack row asked for or not (the buffer always has it).  Data exact without the affine, within one float32 rounding
    of it (ulp of |x scale| + |shift|) otherwise; every margin element of rows < C zero; the slack row zero when asked,
    still NaN when not."""
    lib = _lib()
    rng = np.random.RandomState(M + Cn)
    ld = Cn + 3
    X32 = rng.standard_normal((M, Cn)).astype(np.float32)
    sc32, sh32 = rng.uniform(0.5, 1.5, Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32)
    Xd, scd, shd = padded(X32, ld), dev(sc32), dev(sh32)
    k = 0
    for row_shift in (-T, -1, 0, 1, T - 1):
        for affine in (0, 1):
            for relu in (0, 1):
                for pool in (0, 1):
                    pad, slack = (0, 32, 37)[k % 3], (k // 3) % 2
                    k += 1
                    ldt = M + 2 * pad + 5
                    XT = nans(Cn + 1, ldt)
                    _check(lib.vc_transpose_pad(p(Xd), M, Cn, ld, T, p(scd) if affine else None, p(shd) if affine else None,
                                                relu, pool, row_shift, p(XT), ldt, pad, slack, _st()))
                    got = host(XT)
                    want, bound = R.transpose_pad(f32(X32), T, f32(sc32) if affine else None, f32(sh32) if affine else None,
                                                  relu, pool, row_shift, ldt, pad)
                    what = 'shift %d affine %d relu %d pool %d pad %d slack %d' % (row_shift, affine, relu, pool, pad, slack)
                    _within(got[:Cn, pad:pad + M], want[:, pad:pad + M], bound[:, pad:pad + M], what)
                    assert bool((got[:Cn, :pad] == 0).all()) and bool((got[:Cn, pad + M:] == 0).all()), what + ': margins'
                    assert bool((got[Cn] == 0).all()) if slack else bool(torch.isnan(got[Cn]).all()), what + ': slack row'


# ------------------------------------------------------------------------------------------ filter gradient

MARGIN = 32


def _wgrad_operand(A):
    """[M, C] float32 -> device [(C + 1), M + 2 MARGIN]: transposed, zero margins, one slack row (what vc_transpose_pad
    builds); returns the buffer and the address of frame 0."""
    M, Cn = A.shape
    buf = torch.zeros((Cn + 1, M + 2 * MARGIN), dtype=torch.float32)
    buf[:Cn, MARGIN:MARGIN + M] = torch.from_numpy(A).t()
    buf = buf.cuda()
    return buf, buf.data_ptr() + MARGIN * 4


def _wgrad_run(X32, dY32, T, groups, splits_allowed, outs):
    """groups: (first dY column, N, taps, shift0, index into outs, column offset in that output, ldw)."""
    import _vc
    M, Cin = X32.shape
    XT, x0 = _wgrad_operand(X32)
    YT, y0 = _wgrad_operand(dY32)
    ldt = M + 2 * MARGIN
    d = _vc.WgradDesc()
    d.d_XT = x0
    d.ldxt, d.ldyt, d.Cin, d.M, d.T, d.margin, d.n_groups = ldt, ldt, Cin, M, T, MARGIN, len(groups)
    d.splits_allowed = splits_allowed
    for i, (c0, N, taps, shift0, oi, ocol, ldw) in enumerate(groups):
        g = d.groups[i]
        g.d_dYT = y0 + c0 * ldt * 4
        g.d_dW, g.N, g.taps, g.shift0, g.ldw = outs[oi].data_ptr() + ocol * 4, N, taps, shift0, ldw
    _check(_lib().vc_conv_wgrad(C.byref(d), _st()))
    torch.cuda.synchronize()
    del XT, YT


def _wgrad_inputs(M, Cin, Ntot, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((M, Cin)).astype(np.float32), rng.standard_normal((M, Ntot)).astype(np.float32)


@pytest.mark.parametrize('M,T,Cin,N', [(64, 4, 40, 200), (512, 64, 61, 130), (192, 64, 128, 129)])
def test_wgrad_dense_group_column_slice_and_splits(M, T, Cin, N):
    """vc_conv_wgrad, one dense group (taps = 1) with N not a multiple of the 128-column tile, Cin 40 / 61 (the decoder's
    first dense: 61 of the 64 stored channels) / 128, writing a column slice (ldw) of a wider NaN buffer whose other
    columns must stay NaN.  splits_allowed = 0 twice: bit-identical; splits_allowed = 1 on a pre-zeroed slice (M = 512
    splits the frame range in two: 16 slabs, fewer than 512 blocks).  All against float64, 1e-4 of the maximum."""
    X32, dY32 = _wgrad_inputs(M, Cin, N, M + Cin)
    want = R.wgrad(f32(X32), f32(dY32), T, 1, 0)
    ldw, c0 = N + 11, 5
    runs = []
    for splits in (0, 0, 1):
        out = nans(Cin, ldw)
        if splits:
            out[:, c0:c0 + N] = 0.0
        _wgrad_run(X32, dY32, T, [(0, N, 1, 0, 0, c0, ldw)], splits, [out])
        got = host(out)
        assert bool(torch.isnan(got[:, :c0]).all()) and bool(torch.isnan(got[:, c0 + N:]).all()), 'neighbours written'
        err = _rel_max(got[:, c0:c0 + N], want)
        print('MEASURED wgrad dense M=%d T=%d Cin=%d N=%d splits_allowed=%d err=%.2e bound=1e-4' % (M, T, Cin, N, splits, err))
        assert err < 1e-4, (splits, err)
        runs.append(got[:, c0:c0 + N])
    assert bool((runs[0] == runs[1]).all()), 'fixed summation order: two runs differ'


@pytest.mark.parametrize('M,T,Cin,N', [(64, 4, 40, 40), (512, 64, 128, 130)])
@pytest.mark.parametrize('splits', [0, 1])
def test_wgrad_filter_bank_groups(M, T, Cin, N, splits):
    """Filter-bank groups, taps k = 1 .. 8 with shift0 = -(k / 2) (SAME padding, windows of 4 frames: most taps of the wide
    filters leave the window; and of 64), each group its own slice of dY and its own TF-layout gradient."""
    X32, dY32 = _wgrad_inputs(M, Cin, 8 * N, M + N)
    outs = [torch.zeros((k * Cin, N), dtype=torch.float32, device='cuda') if splits else nans(k * Cin, N) for k in range(1, 9)]
    _wgrad_run(X32, dY32, T, [((k - 1) * N, N, k, -(k // 2), k - 1, 0, 0) for k in range(1, 9)], splits, outs)
    for k in range(1, 9):
        want = R.wgrad(f32(X32), f32(dY32[:, (k - 1) * N:k * N]), T, k, -(k // 2))
        err = _rel_max(host(outs[k - 1]), want)
        assert err < 1e-4, (k, err)


def test_wgrad_xcd_block_map_on_and_off():
    """The XCD-aware block map needs 8 or more groups sorted by taps and 512 or more tiles of 128 rows x 128 columns
    (vc_conv_wgrad in csrc/vc_gemm.hip).  The smallest list that gets there at one column tile per group: 32 groups,
    taps 1 .. 32, Cin = 128: sum k = 528 tiles, over one window of 64 frames; 32 groups also walk both halves of the
    snake that deals groups to XCDs.  Run with the wgrad_xcd option at its default (map on) and 0 (plain grid): both
    against float64, and equal to each other bit for bit (same tiles, same order inside a tile)."""
    import _vc
    M, T, Cin, N = 64, 64, 128, 40
    X32, dY32 = _wgrad_inputs(M, Cin, 32 * N, 3)
    groups = [((k - 1) * N, N, k, -(k // 2), k - 1, 0, 0) for k in range(1, 33)]
    res = []
    try:
        for opt in (-1, 0):
            _vc.set_option('wgrad_xcd', opt)
            outs = [nans(k * Cin, N) for k in range(1, 33)]
            _wgrad_run(X32, dY32, T, groups, 0, outs)
            res.append([host(o) for o in outs])
    finally:
        _vc.set_option('wgrad_xcd', -1)
    for k in range(1, 33):
        want = R.wgrad(f32(X32), f32(dY32[:, (k - 1) * N:k * N]), T, k, -(k // 2))
        for r in res:
            err = _rel_max(r[k - 1], want)
            assert err < 1e-4, (k, err)
        assert bool((res[0][k - 1] == res[1][k - 1]).all()), k


# ------------------------------------------------------------------------------------------ recurrences

def _gru_case(N, T, H, transposed=True):
    lib = _lib()
    rng = np.random.RandomState(N + H + T)
    M = N * T
    xp = f32(rng.standard_normal((M, 6 * H)) * 0.5)
    wh = [f32(rng.standard_normal((H, 3 * H)) * (1.0 / np.sqrt(H))) for _ in range(2)]
    dG = f32(rng.standard_normal((M, 2 * H)))
    xr = xp.clone().requires_grad_(True)
    G_ref, gates_ref, rh_ref = R.gru_train(xr, wh, N, T, H)
    (G_ref * dG).sum().backward()
    xd, w0, w1, dGd = dev(xp), dev(wh[0]), dev(wh[1]), dev(dG)
    G, gates, rh = nans(M, 2 * H), nans(2, M, 3 * H), nans(2, M, H)
    _check(lib.vc_gru_train_forward(p(xd), p(w0), p(w1), N, T, H, p(G), p(gates), p(rh), _st()))
    dpre = nans(M, 6 * H)
    w0t, w1t = (w0.t().contiguous(), w1.t().contiguous()) if transposed else (None, None)
    _check(lib.vc_gru_backward(p(dGd), p(G), p(gates), p(w0), p(w1), p(w0t), p(w1t), N, T, H, p(dpre), _st()))
    e_out = float((host(G) - G_ref.detach()).abs().max())
    e_gates = float((host(gates) - gates_ref.detach()).abs().max())
    e_rh = float((host(rh) - rh_ref.detach()).abs().max())
    e_bwd = _rel_max(host(dpre), xr.grad)
    print('MEASURED gru N=%d T=%d H=%d out=%.2e gates=%.2e rh=%.2e (bound 2e-5) dpre=%.2e (bound 1e-4)' % (N, T, H, e_out, e_gates, e_rh, e_bwd))
    assert e_out < 2e-5 and e_gates < 2e-5 and e_rh < 2e-5, (e_out, e_gates, e_rh)
    assert e_bwd < 1e-4, e_bwd


@pytest.mark.parametrize('N,T,H', [(5, 6, 128), (4, 5, 256), (128, 3, 64), (129, 3, 64), (256, 2, 64), (257, 2, 64),
                                   (3, 7, 30), (2, 4, 61), (2, 3, 520), (1, 1, 40), (3, 1, 128)])
def test_gru_training_pair_dispatch_branches(N, T, H):
    """vc_gru_train_forward / vc_gru_backward, hidden states, ALL saved gates and r*h (2e-5) and d_dpre (1e-4 of its
    maximum) against float64 autograd (train_kernels_ref.gru_train).  Branches: (5,6,128) gru_train_fwd_res_kernel<128> +
    gru_bwd_res_kernel<128>; (4,5,256) gru_train_fwd_res_kernel<256> + gru_bwd_ms_kernel<1>; (128,3,64) the last batch on
    the one-window kernels <1>, (129,3,64) and (256,2,64) <2> (ragged / full last group), (257,2,64) <4> with a group of one;
    (3,7,30) and (2,4,61) the generic kernels (H % 4 != 0); (2,3,520) the generic forward (H above the block of 512) and
    gru_bwd_ms_kernel<1> with more units than threads; (1,1,40) one window of one step, no split of the candidate
    reduction (256 % 40 != 0); (3,1,128) the resident kernels with T = 1."""
    _gru_case(N, T, H)


@pytest.mark.parametrize('N,T,H', [(5, 6, 128), (4, 5, 256)])
def test_gru_training_pair_resident_option_off(N, T, H):
    """gru_train_resident = 0: H = 128 / 256 on gru_train_fwd_ms_kernel<1> / gru_bwd_ms_kernel<1> (weights streamed)."""
    import _vc
    try:
        _vc.set_option('gru_train_resident', 0)
        _gru_case(N, T, H)
    finally:
        _vc.set_option('gru_train_resident', -1)


def test_gru_backward_without_transposed_weights():
    """d_WhT_* NULL: gru_bwd_kernel (generic) at a size the multi-window kernel would otherwise take."""
    _gru_case(3, 9, 64, transposed=False)


@pytest.mark.parametrize('N,T,H', [(1, 1, 24), (3, 7, 72), (2, 5, 128), (3, 4, 130), (2, 3, 512)])
def test_lstm_training_pair(N, T, H):
    """vc_lstm_train_forward / vc_lstm_backward: d_out, activated gates, cell states (2e-5) and d_dpre (1e-4 of its
    maximum) against float64 autograd (train_kernels_ref.lstm_train): one unit-step window, fewer units than a wave
    pair, a whole number of waves, two past it, and H = 512 = the block (every thread owns a unit)."""
    lib = _lib()
    rng = np.random.RandomState(N + H)
    M = N * T
    xp = f32(rng.standard_normal((M, 8 * H)) * 0.5)
    wh = [f32(rng.standard_normal((H, 4 * H)) * (1.0 / np.sqrt(H))) for _ in range(2)]
    dG = f32(rng.standard_normal((M, 2 * H)))
    xr = xp.clone().requires_grad_(True)
    o_ref, g_ref, c_ref = R.lstm_train(xr, wh, N, T, H)
    (o_ref * dG).sum().backward()
    xd, w0, w1, dGd = dev(xp), dev(wh[0]), dev(wh[1]), dev(dG)
    out, gates, cst = nans(M, 2 * H), nans(2, M, 4 * H), nans(2, M, H)
    _check(lib.vc_lstm_train_forward(p(xd), p(w0), p(w1), N, T, H, p(out), p(gates), p(cst), _st()))
    dpre = nans(M, 8 * H)
    w0t, w1t = w0.t().contiguous(), w1.t().contiguous()
    _check(lib.vc_lstm_backward(p(dGd), p(gates), p(cst), p(w0t), p(w1t), N, T, H, p(dpre), _st()))
    errs = [float((host(a) - b.detach()).abs().max()) for a, b in ((out, o_ref), (gates, g_ref), (cst, c_ref))]
    e_bwd = _rel_max(host(dpre), xr.grad)
    print('MEASURED lstm N=%d T=%d H=%d out=%.2e gates=%.2e cstate=%.2e (bound 2e-5) dpre=%.2e (bound 1e-4)' % ((N, T, H) + tuple(errs) + (e_bwd,)))
    assert max(errs) < 2e-5, errs
    assert e_bwd < 1e-4, e_bwd


def test_lstm_training_pair_rejects_513_units():
    import _vc
    lib = _lib()
    t = nans(16)
    with pytest.raises(_vc.VCError, match=r'vc_lstm_train_forward: bad shape n_seq=1 T=1 H=513 \(H <= 512\)'):
        _check(lib.vc_lstm_train_forward(p(t), p(t), p(t), 1, 1, 513, p(t), p(t), p(t), _st()))
    with pytest.raises(_vc.VCError, match=r'vc_lstm_backward: bad shape n_seq=1 T=1 H=513 \(H <= 512\)'):
        _check(lib.vc_lstm_backward(p(t), p(t), p(t), p(t), p(t), 1, 1, 513, p(t), _st()))
    assert bool(torch.isnan(host(t)).all())


# ------------------------------------------------------------------------------------------ reductions

@pytest.mark.parametrize('Cn', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('M', [1, 3, 255, 256, 257, 1000])
def test_col_sum(M, Cn):
    """vc_col_sum: rows around the 256 (64 row blocks x 4 row groups) one pass covers, channels around the 64-column block,
    ld > C with NaN padding; accumulate = 0 over a NaN output, then accumulate = 1 onto known values.  Within 1e-6 of the
    column's sum of magnitudes."""
    lib = _lib()
    rng = np.random.RandomState(M + Cn)
    X32 = rng.standard_normal((M, Cn)).astype(np.float32)
    Xd, ws = padded(X32, Cn + 5), nans(64 * Cn)
    want, mag = R.col_sum(f32(X32))
    out = nans(Cn + 1)
    _check(lib.vc_col_sum(p(Xd), M, Cn, Cn + 5, p(out), 0, p(ws), _st()))
    got = host(out)
    assert bool(torch.isnan(got[Cn:]).all())
    _within(got[:Cn], want, 1e-6 * mag, 'accumulate 0')
    base32 = rng.standard_normal(Cn).astype(np.float32)
    out = torch.cat([dev(base32), nans(1)])
    _check(lib.vc_col_sum(p(Xd), M, Cn, Cn + 5, p(out), 1, p(ws), _st()))
    got = host(out)
    assert bool(torch.isnan(got[Cn:]).all())
    _within(got[:Cn], want + f32(base32), 1e-6 * (mag + f32(base32).abs()), 'accumulate 1')


@pytest.mark.parametrize('rows,Cn,ld', [(1, 1, 2), (51, 5, 8), (65537, 1, 3), (1, 256 * 256 + 3, 256 * 256 + 8)])
def test_mse_loss(rows, Cn, ld):
    """vc_mse_loss with n = 1, 255, 65,537 (one element past one per thread of the 256 x 256 grid) and 256 * 256 + 3; d_dY
    strided with NaN padding that must survive, and d_dY NULL.  Loss within 1e-6 of weight mean(d^2) (a sum of
    non-negative terms: its own sum of magnitudes), d_dY within four float32 roundings."""
    lib = _lib()
    rng = np.random.RandomState(rows + Cn)
    n, w = rows * Cn, 400.0
    y32, t32 = rng.standard_normal((rows, Cn)).astype(np.float32), rng.standard_normal((rows, Cn)).astype(np.float32)
    want, want_d = R.mse_loss(f32(y32), f32(t32), w)
    yd, td, ws = dev(y32), dev(t32), nans(256)
    for with_grad in (True, False):
        dY, loss = nans(rows, ld), nans(2)
        _check(lib.vc_mse_loss(p(yd), p(td), n, w, p(dY) if with_grad else None, Cn, ld, p(loss), p(ws), _st()))
        got = host(loss)
        assert bool(torch.isnan(got[1]))
        assert abs(float(got[0]) - float(want)) <= 1e-6 * float(want), (float(got[0]), float(want))
        gd = host(dY)
        if with_grad:
            assert bool(torch.isnan(gd[:, Cn:]).all())
            _within(gd[:, :Cn], want_d, 4 * EPS32 * want_d.abs(), 'd_dY')
        else:
            assert bool(torch.isnan(gd).all())


@pytest.mark.parametrize('Cn', [1, 61, 64, 65, 130])
@pytest.mark.parametrize('M', [1, 3, 4, 5, 257])
def test_softmax_ce(M, Cn):
    """vc_softmax_ce: rows around the four of a block, classes around the 64 lanes of the wave that owns a row; ldl and
    ldd > C with NaN padding; logits up to +-80; targets whose rows do not sum to 1; exact argmax ties in logits and
    targets (the first index wins on both sides); d_dlogits NULL.  Bounds: the accuracy is exact; a posterior carries the
    rounding of x - max (|x - max| 2^-24), of expf and of the row sum and its reciprocal, together below
    (|x - max| + 16) 2^-24 relative, which bounds d_dlogits element by element (plus two roundings of the target term)
    and, summed over a row, the squared error; the loss is a float32 sum over a row of |t| |x - max| and sum(t) lse
    terms: 1e-6 of their magnitudes."""
    lib = _lib()
    rng = np.random.RandomState(M + Cn)
    x32 = (rng.standard_normal((M, Cn)) * 3).astype(np.float32)
    t32 = rng.uniform(0.0, 1.0, (M, Cn)).astype(np.float32)           # rows sum to about C / 2, not to 1
    x32[0, 0], x32[0, -1] = 80.0, -80.0
    if Cn > 2:
        x32[-1, 1] = x32[-1, 2] = 50.0                                 # tie in the logits
        t32[-1, 1] = t32[-1, 2] = 2.0                                  # and in the target, same place
        if M > 1:
            t32[0, 1] = t32[0, 2] = 2.0                                # target tie against a unique logit maximum
    ldl, ldd = Cn + 3, Cn + 2
    x, t = f32(x32), f32(t32)
    want3, want_d = R.softmax_ce(x, t)
    dmx = (x - x.max(1, keepdim=True).values).abs()
    prob = torch.softmax(x, 1)
    st = t.sum(1, keepdim=True)
    rel_p = (dmx + 16.0) * EPS32
    lse = torch.logsumexp(x - x.max(1, keepdim=True).values, 1, keepdim=True)
    b_loss = 1e-6 * float(((t * dmx).sum(1) + (st * lse.abs())[:, 0]).mean()) + 1e-12
    b_mse = float((2 * (prob - t).abs() * prob * rel_p + 4 * EPS32 * (prob - t) ** 2).mean()) + 1e-12
    xd, td, ws = padded(x32, ldl), dev(t32), nans(3 * M)
    for with_grad in (True, False):
        dl, out3 = nans(M, ldd), nans(4)
        _check(lib.vc_softmax_ce(p(xd), p(td), M, Cn, ldl, p(dl) if with_grad else None, ldd, p(out3), p(ws), _st()))
        got = host(out3)
        assert bool(torch.isnan(got[3]))
        assert abs(float(got[0] - want3[0])) <= b_loss, (float(got[0]), float(want3[0]), b_loss)
        assert abs(float(got[1] - want3[1])) <= EPS32, (float(got[1]), float(want3[1]))
        assert abs(float(got[2] - want3[2])) <= b_mse, (float(got[2]), float(want3[2]), b_mse)
        gd = host(dl)
        if with_grad:
            assert bool(torch.isnan(gd[:, Cn:]).all())
            _within(gd[:, :Cn], want_d, (prob * st * rel_p + 4 * EPS32 * (prob * st + t)) / M, 'd_dlogits')
        else:
            assert bool(torch.isnan(gd).all())


# ------------------------------------------------------------------------------------------ elementwise kernels

@pytest.mark.parametrize('n', [1, 257, BIG_N])
def test_adam_step(n):
    """vc_adam_step with non-zero m and v, grad_scale 0.5, some g = 0, some tiny v; n = 1, one past a block, and past
    the 8,192-block cap (grid-stride loop).  m, v within four roundings (2^-24 each) of their two terms; p, from the m and v
    the device stored, within sixteen (8 ulp) of |p| + |step|: sqrtf and the division are not correctly rounded on the
    device (1 and 2.5 ulp), the product, the sum and the difference add one rounding each.  The element after the last stays NaN."""
    lib = _lib()
    rng = np.random.RandomState(n % 1000)
    p32, g32 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m32, v32 = (rng.standard_normal(n) * 0.1).astype(np.float32), rng.uniform(1e-4, 1e-2, n).astype(np.float32)
    g32[::3] = 0.0
    v32[::5] = 1e-30
    lr_t, b1, b2, eps, gs = (float(np.float32(a)) for a in (3.2e-4, 0.9, 0.999, 1e-8, 0.5))
    wp, wm, wv = R.adam(f32(p32), f32(g32), f32(m32), f32(v32), lr_t, b1, b2, eps, gs)
    bufs = [torch.cat([dev(a), nans(1)]) for a in (p32, m32, v32)]
    gd = dev(g32)
    _check(lib.vc_adam_step(p(bufs[0]), p(gd), p(bufs[1]), p(bufs[2]), n, lr_t, b1, b2, eps, gs, _st()))
    gp, gm, gv = (host(b) for b in bufs)
    for g in (gp, gm, gv):
        assert bool(torch.isnan(g[n]))
    g = f32(g32) * gs
    _within(gm[:n], wm, 4 * EPS32 * ((b1 * f32(m32)).abs() + ((1 - b1) * g).abs()), 'm')
    _within(gv[:n], wv, 4 * EPS32 * (b2 * f32(v32) + (1 - b2) * g * g) + 1e-44, 'v')
    step = lr_t * gm[:n] / (torch.sqrt(gv[:n]) + eps)
    _within(gp[:n], f32(p32) - step, 16 * EPS32 * (f32(p32).abs() + step.abs()), 'p')


@pytest.mark.parametrize('n,Cn', [(37 * 7, 7), (BIG_N, 7)])
def test_affine_act_null_combinations(n, Cn):
    """vc_affine_act with every combination of scale / shift / R given or NULL, relu on and off, C = 7 (does not divide the
    block of 256: the channel of an element changes from block to block); the large n runs the grid-stride loop (there:
    the two extreme combinations only).  Within three float32 roundings (product, sum, sum) of the terms."""
    lib = _lib()
    rng = np.random.RandomState(Cn)
    X32, R32 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    sc32, sh32 = rng.uniform(0.5, 1.5, Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32)
    Xd, Rd, scd, shd = dev(X32), dev(R32), dev(sc32), dev(sh32)
    rows = (n + Cn - 1) // Cn
    tile = lambda v: f32(np.tile(v, rows)[:n])
    combos = [(a, b, c, r) for a in (0, 1) for b in (0, 1) for c in (0, 1) for r in (0, 1)]
    if n == BIG_N:
        combos = [(1, 1, 1, 1), (0, 0, 0, 0)]
    for a, b, c, relu in combos:
        out = nans(n + 1)
        _check(lib.vc_affine_act(p(Xd), p(scd) if a else None, p(shd) if b else None, relu, p(Rd) if c else None, p(out), n, Cn, _st()))
        got = host(out)
        assert bool(torch.isnan(got[n]))
        x = f32(X32)
        want = R.affine_act(x, tile(sc32) if a else None, tile(sh32) if b else None, relu, f32(R32) if c else None)
        mag = ((x * tile(sc32)).abs() if a else x.abs()) * (a | b | c) + tile(sh32).abs() * b + f32(R32).abs() * c
        _within(got[:n], want, 3 * EPS32 * mag, 'scale %d shift %d R %d relu %d' % (a, b, c, relu))


@pytest.mark.parametrize('n', [300, BIG_N])
def test_relu_dropout_backward_and_fill(n):
    """vc_relu_dropout_backward: Y = 0, -0 and a positive denormal among ordinary values (the gradient passes only
    where Y > 0: not through either zero, but through the denormal); vc_fill; both also past the 8,192-block cap."""
    lib = _lib()
    rng = np.random.RandomState(n % 1000)
    Y32 = rng.standard_normal(n).astype(np.float32)
    Y32[0], Y32[1], Y32[2] = 0.0, -0.0, 1e-40
    Y32[-3], Y32[-2], Y32[-1] = 1e-40, -0.0, 0.0
    dY32 = rng.standard_normal(n).astype(np.float32)
    inv_keep = float(np.float32(1.0 / 0.9))
    dZ = nans(n + 1)
    dYd, Yd = dev(dY32), torch.from_numpy(Y32).cuda()
    _check(lib.vc_relu_dropout_backward(p(dYd), p(Yd), inv_keep, p(dZ), n, _st()))
    got = host(dZ)
    want = R.relu_dropout_backward(f32(dY32), torch.from_numpy(Y32), inv_keep)
    assert bool(torch.isnan(got[n]))
    assert float(want[2]) != 0.0 and float(want[0]) == 0.0 and float(want[1]) == 0.0
    _within(got[:n], want, EPS32 * want.abs(), 'dZ')
    buf = nans(n + 1)
    _check(lib.vc_fill(p(buf), 0.25, n, _st()))
    got = host(buf)
    assert bool((got[:n] == 0.25).all()) and bool(torch.isnan(got[n]))


@pytest.mark.parametrize('H', [32, 40, 72, 128])
def test_highway_backward(H):
    """vc_highway_backward in the paired layout; for NP != 2H (H = 40, 72) the padding columns of d_dpre come out zero;
    a wrong NP is rejected before any launch.  The gate is 1 / (1 + __expf(-v)): the fast exponential rounds v log2(e)
    (|v| 2^-24 relative, |v| < 6 here) and the hardware exp2 and reciprocal add a rounding or two each, the products
    three more: bound 2e-6 of |dO| max(1, |h - x|)."""
    import _vc
    lib = _lib()
    rng = np.random.RandomState(H)
    M, NP = 70, 64 * ((H + 31) // 32)
    pre32 = rng.standard_normal((M, NP)).astype(np.float32)
    X32, dO32 = rng.standard_normal((M, H)).astype(np.float32), rng.standard_normal((M, H)).astype(np.float32)
    dpre, dXd = nans(M, NP), nans(M, H)
    pred, Xd, dOd = dev(pre32), dev(X32), dev(dO32)
    _check(lib.vc_highway_backward(p(pred), NP, p(Xd), p(dOd), M, H, p(dpre), p(dXd), _st()))
    want_p, want_x = R.highway_backward(f32(pre32), f32(X32), f32(dO32), H)
    ch, ct = R.paired_columns(H)
    mag = f32(dO32).abs() * torch.clamp((torch.clamp(f32(pre32)[:, ch], min=0.0) - f32(X32)).abs(), min=1.0)
    bound = torch.zeros_like(want_p)
    bound[:, ch] = 2e-6 * mag
    bound[:, ct] = 2e-6 * mag
    _within(host(dpre), want_p, bound, 'd_dpre')
    _within(host(dXd), want_x, 2e-6 * mag, 'd_dXd')
    with pytest.raises(_vc.VCError, match='NP must be the paired width'):
        _check(lib.vc_highway_backward(p(dpre), 2 * H + 1, p(dXd), p(dXd), M, H, p(dpre), p(dXd), _st()))


def test_axpby_strides_and_aliasing():
    """vc_axpby with three different row strides, then with out aliasing X and out aliasing Y; padding columns of the
    output untouched.  Within two float32 roundings of the two terms."""
    lib = _lib()
    rng = np.random.RandomState(4)
    M, Cn, a, b = 37, 13, float(np.float32(0.3)), float(np.float32(-1.7))
    X32, Y32 = rng.standard_normal((M, Cn)).astype(np.float32), rng.standard_normal((M, Cn)).astype(np.float32)
    want = R.axpby(a, f32(X32), b, f32(Y32))
    bound = 2 * EPS32 * ((a * f32(X32)).abs() + (b * f32(Y32)).abs())
    for alias in (None, 'X', 'Y'):
        Xd, Yd = padded(X32, Cn + 2), padded(Y32, Cn + 5)
        out = {None: nans(M, Cn + 9), 'X': Xd, 'Y': Yd}[alias]
        ldo = out.shape[1]
        _check(lib.vc_axpby(p(Xd), Cn + 2, a, p(Yd), Cn + 5, b, p(out), ldo, M, Cn, _st()))
        got = host(out)
        assert bool(torch.isnan(got[:, Cn:]).all()), alias
        _within(got[:, :Cn], want, bound, 'alias %s' % alias)
