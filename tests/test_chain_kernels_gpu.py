"""The fused chain launches alone, through the C ABI: vc_mfma_pack, vc_prenet_chain (both kernel forms) and vc_cbhg_front of
csrc/vc_cbhg_small.hip, vc_highway_pack and vc_highway_chain of csrc/vc_highway.hip, against the float64 definitions of
tests/chain_ref.py on the inputs of tests/chain_cases.py (tests/test_chain_kernels_cpu.py proves those usable).  The tests
pack their own weights with the library's pack launches and build their own coefficient table.

Every test starts with poison_gpu_state(); every launch runs twice and the raw bits must agree; outputs start as NaN with a
fixed payload, which must survive in every gap (ld > width) and behind every buffer; input gaps hold NaN.
Exact cases are compared bit for bit.  Real-valued cases are held to the bound chain_ref derives element by element,
with the device gate's own error at 4 x GATE_MAX; a line starting with MEASURED carries error, bound and their largest
ratio (profiles/chain_kernels/README.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_cases as Cs
import chain_ref as R
import conv_gemm_ref as G
from conftest import poison_gpu_state
from test_chain_kernels_cpu import _oracle_weights

pytestmark = pytest.mark.gpu

GATE_MAX = Cs.GATE_MAX
GATE_ERR = 4 * GATE_MAX
VC_ERR_INVALID = 1
NAN16, NAN32 = 0x7FA5, 0x7FA5A5A5          # the canaries: NaN with a payload no arithmetic produces
BF16, F32 = torch.bfloat16, torch.float32


def _lib():
    import _vc
    return _vc.lib()


def _st():
    import _vc
    return _vc.current_stream()


def _ok(rc):
    import _vc
    _vc.check(rc)
    torch.cuda.synchronize()


def _refused(rc, text):
    msg = _lib().vc_last_error().decode()
    assert rc == VC_ERR_INVALID and text in msg, (rc, msg, text)


@pytest.fixture(autouse=True)
def _default_options():
    import _vc
    yield
    for n in ('prenet_lds', 'cbhg_front_mi'):
        _vc.set_option(n, -1)


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def dev16(a):
    """float64 on the bf16 grid -> device bf16."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    assert np.array_equal(R.to_bf16(a), a.astype(np.float64)), 'not on the bf16 grid'
    return torch.from_numpy(a).bfloat16().cuda()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def rows_in(a, ld, dtype):
    """[M, C] -> device [M, ld] of dtype, NaN in the gap."""
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[0], ld), float('nan'), dtype=torch.float64)
    t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a))
    if dtype == BF16:
        assert np.array_equal(R.to_bf16(a), a, equal_nan=True), 'not on the bf16 grid'
    return t.to(dtype).cuda()


class Out:
    """An output of rows x width elements at pitch ld, followed by 256 more elements: canaries everywhere."""

    def __init__(self, rows, width, ld, dtype, start=None):
        self.rows, self.width, self.ld, self.dtype = rows, width, ld, dtype
        self.idt, self.can = (torch.int16, NAN16) if dtype == BF16 else (torch.int32, NAN32)
        self.raw = torch.full((rows * ld + 256,), self.can, dtype=self.idt, device='cuda')
        self.t = self.raw.view(dtype)
        if start is not None:                            # in-place launches: the input's bits inside the rows
            self.raw[:rows * ld].view(rows, ld)[:, :width] = start.view(self.idt)[:, :width]

    def bits(self):
        """The rows' bits on the host; gaps and tail must still hold the canary."""
        torch.cuda.synchronize()
        body = self.raw[:self.rows * self.ld].view(self.rows, self.ld)
        assert bool((body[:, self.width:] == self.can).all()), 'wrote into the gap between rows'
        assert bool((self.raw[self.rows * self.ld:] == self.can).all()), 'wrote behind the buffer'
        return body[:, :self.width].cpu().numpy().copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == self.can).all())


def bits_of(v, dtype):
    """Expected float64 values -> the bits the device must store."""
    v = np.asarray(v, dtype=np.float32)
    if dtype == BF16:
        assert np.array_equal(R.to_bf16(v), v.astype(np.float64))
        return R.to_bf16_bits(v).view(np.int16)
    return v.view(np.int32)


def values_of(bits, dtype):
    if dtype == BF16:
        return R.from_bf16_bits(bits.view(np.uint16)).astype(np.float64)
    return bits.view(np.float32).astype(np.float64)


def same_bits(got, want, what):
    """Bit for bit, signed zeros alike (the kernels' relu returns +0 where float64 max keeps the sign of what it was given)."""
    if not np.array_equal(got, want):
        g, w = values_of(got, BF16 if got.dtype == np.int16 else F32), values_of(want, BF16 if want.dtype == np.int16 else F32)
        bad = np.argwhere(~(g == w))
        assert bad.size == 0, '%s: %d of %d elements differ, first at %s: got %r, expected %r' % (
            what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


def measured(what, got, ref):
    err = np.abs(got - ref.v)
    ratio = float((err / ref.e).max())
    print('MEASURED %s err=%.3e bound=%.3e err/bound=%.3f' % (what, float(err.max()), float(ref.e.max()), ratio))
    return ratio


def twice(run, what):
    """run() -> Out (or tuple of Out): two launches into fresh canaries, identical bits; the first one's bits."""
    a, b = run(), run()
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    first = tuple(None if o is None else o.bits() for o in a)
    for x, o in zip(first, b):
        if o is not None:
            assert np.array_equal(x, o.bits()), what + ': two launches differ'
    return first if len(first) > 1 else first[0]


# ------------------------------------------------------------------------------------------ the pack launches

def mfma_pack(W, rows, K, chained, ldw=None):
    """vc_mfma_pack of a float64 matrix on the bf16 grid (ldw > K: NaN in the padding) -> device bf16 fragments."""
    ldw = ldw or W.shape[1]
    src = rows_in(np.asarray(W)[:rows, :K], ldw, BF16)
    out = Out(1, ((rows + 31) // 32) * ((K + 15) // 16) * 512, ((rows + 31) // 32) * ((K + 15) // 16) * 512, BF16)
    _ok(_lib().vc_mfma_pack(ptr(src), rows, K, ldw, chained, ptr(out.t), _st()))
    return out, src


def highway_pack(Bt, H):
    src = dev16(Bt)
    out = Out(1, src.numel(), src.numel(), BF16)
    _ok(_lib().vc_highway_pack(ptr(src), Bt.shape[0], H, ptr(out.t), _st()))
    return out, src


def test_mfma_pack_is_the_index_formula_bit_for_bit():
    """rows and K at 1, on both sides of the 32-row tile and the 16-wide k-step, the front's own shapes and conv1d_1's
    2304; ldw > K with NaN in the padding; plain and chained; zero fill outside W; nothing behind the output."""
    poison_gpu_state()
    rng = np.random.RandomState(3)
    for rows in (1, 31, 32, 33, 40, 240):
        for K in (1, 15, 16, 17, 40, 120, 240, 2304):
            W = R.from_bf16_bits(rng.randint(0x3c00, 0x4400, (rows, K)).astype(np.uint16) | (rng.randint(0, 2, (rows, K)) << 15).astype(np.uint16)).astype(np.float64)
            for chained in (0, 1):
                for ldw in ((K, K + 8) if chained == 0 else (K + 1,)):
                    got = twice(lambda: mfma_pack(W, rows, K, chained, ldw)[0], 'vc_mfma_pack')
                    want = R.mfma_pack(R.to_bf16_bits(W).view(np.int16), rows, K, chained)
                    assert np.array_equal(got.reshape(-1), want), (rows, K, chained, ldw)


def test_highway_pack_is_the_index_formula_bit_for_bit():
    poison_gpu_state()
    rng = np.random.RandomState(4)
    for H in (128, 256):
        for n in (64, 2 * H, 6 * H):
            Bt = R.from_bf16_bits(rng.randint(0x3c00, 0x4400, (n, H)).astype(np.uint16)).astype(np.float64)
            got = twice(lambda: highway_pack(Bt, H)[0], 'vc_highway_pack')
            assert np.array_equal(got.reshape(-1), R.highway_pack(R.to_bf16_bits(Bt).view(np.int16), H)), (H, n)


def test_pack_launches_refuse_bad_arguments():
    poison_gpu_state()
    lib, st = _lib(), _st()
    W = dev16(np.ones((64, 256)))
    out = Out(1, 64 * 256, 64 * 256, BF16)
    for args in ((None, 32, 16, 16, 0, ptr(out.t)), (ptr(W), 32, 16, 16, 0, None), (ptr(W), 0, 16, 16, 0, ptr(out.t)),
                 (ptr(W), 32, 0, 16, 0, ptr(out.t)), (ptr(W), -1, 16, 16, 0, ptr(out.t)), (ptr(W), 32, 17, 16, 0, ptr(out.t))):
        _refused(lib.vc_mfma_pack(*args, st), 'vc_mfma_pack: bad argument')
    for args in ((None, 64, 256, ptr(out.t)), (ptr(W), 64, 256, None), (ptr(W), 64, 64, ptr(out.t)), (ptr(W), 64, 192, ptr(out.t)),
                 (ptr(W), 0, 256, ptr(out.t)), (ptr(W), -64, 256, ptr(out.t)), (ptr(W), 32, 256, ptr(out.t)), (ptr(W), 96, 128, ptr(out.t))):
        _refused(lib.vc_highway_pack(*args, st), 'vc_highway_pack: H must be 128 or 256')
    assert out.untouched()


# ------------------------------------------------------------------------------------------ vc_prenet_chain

class Prenet:
    def __init__(self, shape, kind):
        self.shape = shape
        cin, u1, u2 = shape
        self.w = Cs.prenet_weights(shape, kind)
        W1, b1, W2, b2 = self.w
        self.pk1, _ = mfma_pack(W1, u1, cin, 0)
        self.pk2, _ = mfma_pack(W2, u2, u1, 1)
        self.b1, self.b2 = dev32(b1), dev32(b2)

    def launch(self, X, x_f32, ldx, ldy):
        cin, u1, u2 = self.shape
        M = X.shape[0]
        xd = rows_in(X, ldx, F32 if x_f32 else BF16)
        out = Out(M, u2, ldy, BF16)
        _ok(_lib().vc_prenet_chain(ptr(xd), x_f32, M, ldx, cin, u1, u2, ptr(self.pk1.t), ptr(self.b1), ptr(self.pk2.t), ptr(self.b2),
                                   ptr(out.t), ldy, _st()))
        return out

    def both_forms(self, X, x_f32, ldx, ldy, what):
        import _vc
        res = []
        for form in (-1, 0):
            _vc.set_option('prenet_lds', form)
            res.append(twice(lambda: self.launch(X, x_f32, ldx, ldy), what))
        _vc.set_option('prenet_lds', -1)
        assert np.array_equal(res[0], res[1]), what + ': the LDS form and the per-wave form differ'
        return res[0]


@pytest.mark.parametrize('shape', Cs.PRENET_SHAPES, ids=lambda s: '%d-%d-%d' % s)
def test_prenet_chain_exact_cases_bit_for_bit(shape):
    """One-hot rows (every dense1 weight observed singly; bf16 and float32 features), rows of several ones, and float32
    one-hot rows on bf16 ties that round down (to 1) and up (to 2); M = 1 .. 257 around the 32-row wave tile and the
    128-row block; ldx and ldy wider than the rows; both kernel forms, bit-identical to each other."""
    poison_gpu_state()
    cin, u1, u2 = shape
    nets = {k: Prenet(shape, k) for k in ('onehot', 'ints')}
    for inp, wk, xf in Cs.PRENET_EXACT:
        W1, b1, W2, b2 = nets[wk].w
        for M in Cs.PRENET_M:
            X = Cs.prenet_input(shape, inp, M)
            want = bits_of(R.prenet(X, W1, b1, W2, b2, xf).v, BF16)
            for ldx, ldy in ((cin, u2), (cin + 8, u2 + 8)):
                got = nets[wk].both_forms(X, xf, ldx, ldy, 'prenet %s M=%d' % (inp, M))
                same_bits(got, want, 'prenet %s M=%d x_f32=%d ldx=%d ldy=%d' % (inp, M, xf, ldx, ldy))


@pytest.mark.parametrize('shape', Cs.PRENET_SHAPES, ids=lambda s: '%d-%d-%d' % s)
def test_prenet_chain_real_valued_within_the_derived_bound_and_equal_to_two_dense_launches(shape):
    """Real-valued data under chain_ref's bound (both feature types), and against two vc_conv_gemm launches (dense + relu,
    bf16 between them) at every M of the list: the header promised 'bit-identical in practice, tested to 1e-2'; measured
    on the device it IS bit-identical at all of them, so equality is what is asserted."""
    from test_conv_gemm_gpu import Launch
    poison_gpu_state()
    cin, u1, u2 = shape
    net = Prenet(shape, 'real')
    W1, b1, W2, b2 = net.w
    worst = 0
    for M in Cs.PRENET_M:
        X = Cs.prenet_input(shape, 'real', M)
        for xf in (0, 1):
            Xf = X + (2.0 ** -10 if xf else 0.0) * np.sign(X)              # float32 features off the bf16 grid
            ref = R.prenet(Xf, W1, b1, W2, b2, xf)
            got = net.both_forms(Xf, xf, cin + 8, u2 + 8, 'prenet real M=%d' % M)
            assert measured('prenet %d-%d-%d M=%d x_f32=%d' % (cin, u1, u2, M, xf), values_of(got, BF16), ref) <= 1.0
        d1 = G.desc(X, M, u1, [G.group(W1, 1, 0, 0)], dtype=G.BF16, epi_shift=b1, act=G.ACT_RELU)
        y1 = Launch(d1, cin).run()
        d2 = G.desc(y1.float().cpu().double().numpy(), M, u2, [G.group(W2, 1, 0, 0)], dtype=G.BF16, epi_shift=b2, act=G.ACT_RELU)
        two = Launch(d2, u1).run().view(torch.int16).cpu().numpy()
        one = twice(lambda: net.launch(X, 0, cin, u2), 'prenet')
        diff = int((one != two).sum())
        worst = max(worst, diff)
        print('MEASURED prenet %d-%d-%d M=%d against two vc_conv_gemm launches: %d of %d elements differ' % (cin, u1, u2, M, diff, one.size))
    assert worst == 0


def test_prenet_chain_refuses_bad_arguments():
    poison_gpu_state()
    lib, st = _lib(), _st()
    net = Prenet((64, 256, 128), 'ints')
    X16, X32 = rows_in(np.zeros((4, 72)), 72, BF16), rows_in(np.zeros((4, 72)), 72, F32)
    out = Out(4, 128, 136, BF16)
    good = dict(X=ptr(X16), xf=0, M=4, ldx=64, cin=64, u1=256, u2=128, pk1=ptr(net.pk1.t), b1=ptr(net.b1), pk2=ptr(net.pk2.t), b2=ptr(net.b2),
                Y=ptr(out.t), ldy=128)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vc_prenet_chain(a['X'], a['xf'], a['M'], a['ldx'], a['cin'], a['u1'], a['u2'], a['pk1'], a['b1'], a['pk2'], a['b2'], a['Y'], a['ldy'], st)
    for k in ('X', 'pk1', 'b1', 'pk2', 'b2', 'Y'):
        _refused(call(**{k: None}), 'NULL argument or M <= 0')
    for M in (0, -1):
        _refused(call(M=M), 'NULL argument or M <= 0')
    for cin, u1, u2 in ((64, 256, 256), (80, 256, 128), (64, 512, 256), (72, 256, 128), (80, 512, 128)):
        _refused(call(cin=cin, u1=u1, u2=u2, ldx=80), 'unsupported shape')
    for kw in (dict(ldx=56), dict(ldx=68), dict(X=ptr(X32), xf=1, ldx=66), dict(ldy=120), dict(ldy=132)):
        _refused(call(**kw), 'leading dimensions')
    for k, t in (('X', X16), ('Y', out.t), ('pk1', net.pk1.t), ('pk2', net.pk2.t), ('b1', net.b1), ('b2', net.b2)):
        _refused(call(**{k: ptr(t, 8)}), '16-byte aligned')
    assert out.untouched()
    assert lib.vc_prenet_chain_supported(64, 256, 128) and lib.vc_prenet_chain_supported(80, 512, 256)
    assert not lib.vc_prenet_chain_supported(64, 512, 256) and not lib.vc_prenet_chain_supported(80, 256, 128)
    _ok(call(X=ptr(X32), xf=1, ldx=68))                  # float32 rows need a multiple of 4 only


# ------------------------------------------------------------------------------------------ vc_highway_chain

class Highway:
    def __init__(self, H, kind):
        self.H = H
        self.layers, self.tail = Cs.highway_weights(H, kind)
        self.pk = [highway_pack(Wp, H)[0] for Wp, _ in self.layers]
        self.bias = [dev32(bp) for _, bp in self.layers]
        self.ppk = {n: highway_pack(self.tail[0][:n], H)[0] for n in Cs.highway_tails(H)}
        self.pb = dev32(self.tail[1])

    def launch(self, X, L, form, n_proj=0, wide=False):
        """form 'Y': d_Y separate; 'inplace': d_Y == d_X; 'tail': d_Y NULL with a tail; 'both'.  -> (Y Out or None, P Out or None)"""
        H, M = self.H, X.shape[0]
        ldx = H + 8 if wide else H
        xd = rows_in(X, ldx, BF16)
        if form == 'inplace':
            Y = Out(M, H, ldx, BF16, start=xd)
            xp = yp = ptr(Y.t)
        else:
            Y = Out(M, H, ldx, BF16) if form in ('Y', 'both') else None
            xp, yp = ptr(xd), None if Y is None else ptr(Y.t)
        P = None
        ldp = n_proj + 4 if wide else n_proj
        if n_proj:
            P = Out(M, n_proj, ldp, F32)
        PA = (C.c_void_p * max(L, 1))(*[o.t.data_ptr() for o in self.pk[:L]])
        BA = (C.c_void_p * max(L, 1))(*[b.data_ptr() for b in self.bias[:L]])
        _ok(_lib().vc_highway_chain(xp, M, H, ldx, L, PA, BA, yp, ldx if Y is not None else 0,
                                    ptr(self.ppk[n_proj].t) if n_proj else None, ptr(self.pb) if n_proj else None, n_proj,
                                    None if P is None else ptr(P.t), ldp, _st()))
        return Y, P

    def forms(self):
        nw64 = Cs.highway_tails(self.H)
        return [('Y', 0, False), ('Y', 0, True), ('inplace', 0, True)] + [('tail', n, n != nw64[3]) for n in nw64] + [('both', nw64[2], False)]


@pytest.fixture(scope='module')
def highway_nets():
    return {}


def _net(cache, H, kind):
    if (H, kind) not in cache:
        cache[(H, kind)] = Highway(H, kind)
    return cache[(H, kind)]


@pytest.mark.parametrize('L', Cs.HIGHWAY_LAYERS)
@pytest.mark.parametrize('H', Cs.HIGHWAY_H)
def test_highway_chain_exact_cases_bit_for_bit(highway_nets, H, L):
    """Identity rows (M = H: every dense1 and dense2 weight of the first layer observed singly, gates of exactly 0, 1/2 and 1)
    and sparse integer rows at M = 1, 127, 128, 129, 300; 0, 1, 2 and 8 layers (0 without a tail: a copy); d_Y separate, in
    place, absent; tails of 64, 64 NW, 64 (NW + 1) and 6H columns; ldx, ldy, ldp wider than the rows."""
    poison_gpu_state()
    net = _net(highway_nets, H, 'exact')
    for M in sorted(set(Cs.HIGHWAY_M) | {H}):
        X, Y, P, _ = Cs.highway_case(H, 'exact', L, M)
        for form, n_proj, wide in net.forms():
            what = 'highway H=%d L=%d M=%d %s n_proj=%d wide=%d' % (H, L, M, form, n_proj, wide)
            y, pr = twice(lambda: net.launch(X, L, form, n_proj, wide), what)
            if y is not None:
                same_bits(y, bits_of(Y.v, BF16), what + ' (Y)')
            if pr is not None:
                same_bits(pr, bits_of(P.v[:, :n_proj], F32), what + ' (P)')


@pytest.mark.parametrize('L', Cs.HIGHWAY_LAYERS)
@pytest.mark.parametrize('H', Cs.HIGHWAY_H)
def test_highway_chain_real_valued_within_the_derived_bound(highway_nets, H, L):
    poison_gpu_state()
    net = _net(highway_nets, H, 'real')
    for M in Cs.HIGHWAY_M:
        X, Y, P, _ = Cs.highway_case(H, 'real', L, M, GATE_ERR)
        n = Cs.highway_tails(H)
        for form, n_proj in (('both', n[3]), ('tail', n[0]), ('inplace', 0)):
            y, pr = twice(lambda: net.launch(X, L, form, n_proj, True), 'highway real')
            if y is not None and L:
                assert measured('highway H=%d L=%d M=%d Y(bf16)' % (H, L, M), values_of(y, BF16), Y) <= 1.0
            elif y is not None:
                same_bits(y, bits_of(X, BF16), 'a chain of no layers copies')
            if pr is not None:
                ref = R.Tracked(P.v[:, :n_proj], P.e[:, :n_proj])
                assert measured('highway H=%d L=%d M=%d tail(f32, %d)' % (H, L, M, n_proj), values_of(pr, F32), ref) <= 1.0


@pytest.mark.parametrize('H', Cs.HIGHWAY_H)
def test_highway_chain_equals_the_per_layer_launches(highway_nets, H):
    """8 layers and the 6H tail in one launch against eight vc_conv_gemm(VC_GEMM_HIGHWAY) launches and a dense one."""
    from test_conv_gemm_gpu import Launch
    poison_gpu_state()
    net = _net(highway_nets, H, 'real')
    M = 300
    X = Cs.highway_input(H, 'real', M)
    y, pr = twice(lambda: net.launch(X, 8, 'both', 6 * H), 'highway')
    x = X
    for Wp, bp in net.layers:
        d = G.desc(x, M, 2 * H, [G.group(Wp, 1, 0, 0)], dtype=G.BF16, mode=G.HIGHWAY, epi_shift=bp)
        t = Launch(d, H).run()
        x = t.float().cpu().double().numpy()
    assert np.array_equal(t.view(torch.int16).cpu().numpy(), y)
    d = G.desc(x, M, 6 * H, [G.group(net.tail[0], 1, 0, 0)], dtype=G.BF16, epi_shift=net.tail[1], out_f32=1)
    assert np.array_equal(Launch(d, H).run().view(torch.int32).cpu().numpy(), pr)


def test_highway_gate_alone():
    """vc::highway_gate (exp2 of -x log2 e, rcp of 1 + that, one fma) has no derived error.  The chain kernels store bf16, so
    the same device function is observed through vc_conv_gemm's highway mode with a float32 output: transform weights pick
    a coarse bf16 number (multiples of 1/4 in [-20, 20]) from the upper half of the row, the float32 bias adds a multiple of
    1/256 (the sum is exact), dense1 is 0 with a bias of 1 and the carried input 0, so the output IS the device's sigmoid.
    Held to 4 x the recorded maximum."""
    from test_conv_gemm_gpu import Launch
    assert GATE_ERR <= 2e-5
    poison_gpu_state()
    H = 128
    coarse = np.arange(-80, 81) / 4.0
    X = np.zeros((len(coarse), H))
    X[:, 64:] = coarse[:, None]
    W1, W2 = np.zeros((H, H)), np.zeros((H, H))
    W2[np.arange(64), np.arange(64) + 64] = 1.0
    b1, b2 = np.zeros(H), np.zeros(H)
    b1[:64], b2[:64] = 1.0, np.arange(64) / 256.0
    Wp, bp = R.pair(W1, b1, W2, b2)
    d = G.desc(X, len(coarse), 2 * H, [G.group(Wp, 1, 0, 0)], dtype=G.BF16, mode=G.HIGHWAY, epi_shift=bp, out_f32=1)
    L = Launch(d, H)
    a, b = L.run(), L.run()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = a.cpu().double().numpy()[:, :64]
    tpre = coarse[:, None] + b2[None, :64]
    err = float(np.abs(got - R.sigmoid(tpre)).max())
    print('MEASURED highway_gate sigmoid max|err|=%.3e over %d pre-activations in [-20, 20.25) (recorded %.1e)' % (err, tpre.size, GATE_MAX))
    assert err <= GATE_ERR
    # the pinned gates of the exact cases: exactly 1/2, 1 and 0
    X = np.zeros((8, H))
    b2 = np.zeros(H)
    b2[:3] = (0.0, 2048.0, -2048.0)
    Wp, bp = R.pair(np.zeros((H, H)), b1, np.zeros((H, H)), b2)
    d = G.desc(X, 8, 2 * H, [G.group(Wp, 1, 0, 0)], dtype=G.BF16, mode=G.HIGHWAY, epi_shift=bp, out_f32=1)
    assert Launch(d, H).run().cpu().numpy()[0, :3].tolist() == [0.5, 1.0, 0.0]


def test_highway_chain_refuses_bad_arguments(highway_nets):
    poison_gpu_state()
    lib, st = _lib(), _st()
    net = _net(highway_nets, 128, 'exact')
    H, M = 128, 4
    X = rows_in(np.zeros((M, H)), H + 8, BF16)
    Y, P = Out(M, H, H + 8, BF16), Out(M, 64, 68, F32)
    PA = (C.c_void_p * 8)(*[o.t.data_ptr() for o in net.pk])
    BA = (C.c_void_p * 8)(*[b.data_ptr() for b in net.bias])
    good = dict(X=ptr(X), M=M, H=H, ldx=H, L=2, PA=PA, BA=BA, Y=ptr(Y.t), ldy=H, PW=ptr(net.ppk[64].t), pb=ptr(net.pb), NP=64, P=ptr(P.t), ldp=64)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vc_highway_chain(a['X'], a['M'], a['H'], a['ldx'], a['L'], a['PA'], a['BA'], a['Y'], a['ldy'], a['PW'], a['pb'], a['NP'], a['P'], a['ldp'], st)
    for kw in (dict(X=None), dict(PA=None), dict(BA=None), dict(Y=None, PW=None)):
        _refused(call(**kw), 'NULL argument')
    for kw in (dict(pb=None), dict(P=None), dict(NP=0), dict(NP=96), dict(NP=-64), dict(ldp=60), dict(ldp=66), dict(PW=ptr(net.ppk[64].t, 8)),
               dict(pb=ptr(net.pb, 4)), dict(P=ptr(P.t, 8))):
        _refused(call(**kw), 'projection tail needs')
    for Hbad in (64, 192, 512, 0):
        _refused(call(H=Hbad), 'H must be 128 or 256')
    for kw in (dict(M=0), dict(M=-3), dict(L=-1), dict(L=9)):
        _refused(call(**kw), 'bad M / n_layers')
    for kw in (dict(ldx=120), dict(ldx=132), dict(ldy=120), dict(ldy=132)):
        _refused(call(**kw), 'ldx / ldy')
    for kw in (dict(X=ptr(X, 8)), dict(Y=ptr(Y.t, 8))):
        _refused(call(**kw), 'X / Y must be 16-byte aligned')
    for i, arr in ((1, 'PA'), (0, 'BA')):
        bad = (C.c_void_p * 8)(*[(o.t if arr == 'PA' else o).data_ptr() for o in (net.pk if arr == 'PA' else net.bias)])
        bad[i] = None
        _refused(call(**{arr: bad}), 'layer %d operands NULL or misaligned' % i)
        bad[i] = (net.pk[i].t if arr == 'PA' else net.bias[i]).data_ptr() + 8
        _refused(call(**{arr: bad}), 'layer %d operands NULL or misaligned' % i)
    assert Y.untouched() and P.untouched()


# ------------------------------------------------------------------------------------------ vc_cbhg_front

class Front:
    """The packed weights and coefficient table of one weight set, packed by the library's own launch."""

    def __init__(self, p):
        import _vc
        self.p = p
        self.keep = []
        d = _vc.CbhgFrontDesc()
        for name, W, rows, K, chained in R.front_packed(p):
            o, _ = mfma_pack(W, rows, K, chained, ldw=K + 8)
            self.keep.append(o)
            setattr(d, name, o.t.data_ptr())
        self.bank = torch.cat([mfma_pack(b, R.FILTERS, R.WIDTH * (k + 1), 0)[0].t[:4 * ((R.WIDTH * (k + 1) + 15) // 16) * 512] for k, b in enumerate(p['bank'])])
        d.d_pk_bank = self.bank.data_ptr()
        for l, (Wp, _) in enumerate(p['hw']):
            o, _ = mfma_pack(Wp, 128, R.WIDTH, 1)
            self.keep.append(o)
            d.d_pk_highway[l] = o.t.data_ptr()
        co = R.coef_table(p)
        assert len(co) == _lib().vc_cbhg_front_coef_floats()
        self.coef = dev32(co)
        d.d_coef = self.coef.data_ptr()
        d.n_features, d.prenet_units, d.width, d.n_banks, d.bank_filters, d.gru_units = R.FEAT, R.UNITS, R.WIDTH, R.BANKS, R.FILTERS, R.GRU
        d.n_highway = len(p['hw'])
        self.d = d

    def launch(self, X, n, T, x_f32, wide=True, expect=None):
        ldx, ldp = (R.FEAT + 8, 6 * R.GRU + 4) if wide else (R.FEAT, 6 * R.GRU)
        xd = rows_in(X, ldx, F32 if x_f32 else BF16)
        out = Out(n * T, 6 * R.GRU, ldp, F32)
        d = self.d
        d.d_x, d.x_f32, d.ldx, d.n_windows, d.T, d.d_xproj, d.ldp = xd.data_ptr(), x_f32, ldx, n, T, out.t.data_ptr(), ldp
        _ok(_lib().vc_cbhg_front(C.byref(d), _st()))
        return out


@pytest.fixture(scope='module')
def fronts():
    return {}


def _front(cache, kind, L):
    if (kind, L) not in cache:
        cache[(kind, L)] = Front(Cs.front_weights(kind, L))
    return cache[(kind, L)]


@pytest.mark.parametrize('mi', [2, 4])
def test_cbhg_front_exact_cases_bit_for_bit(fronts, mi):
    """xproj itself, bit for bit: every listed window length (one tile, one frame into the next tile, a short last tile) at
    1 and 3 windows, bf16 features and float32 features on rounding ties, no highway layers; 1 and 4 highway layers with
    gates pinned at 1/2, 1 and 0 at the two longest windows.  Random sparse integers give every frame, filter width, tap,
    channel slice and coefficient slot its own value (tests/test_chain_kernels_cpu.py shows each layout mix-up changes the
    result); all bank shifts are non-zero."""
    import _vc
    poison_gpu_state()
    _vc.set_option('cbhg_front_mi', mi)
    for L, n, T, xf in Cs.front_exact_list(mi):
        X, xproj, _ = Cs.front_case('exact', L, n, T, xf)
        what = 'front mi=%d L=%d n=%d T=%d x_f32=%d' % (mi, L, n, T, xf)
        got = twice(lambda: _front(fronts, 'exact', L).launch(X, n, T, xf), what)
        same_bits(got, bits_of(xproj.v, F32), what)


@pytest.mark.parametrize('mi', [2, 4])
def test_cbhg_front_real_valued_within_the_derived_bound(fronts, mi):
    import _vc
    poison_gpu_state()
    _vc.set_option('cbhg_front_mi', mi)
    for L, n, T, xf in Cs.front_real_list(mi):
        X, xproj, _ = Cs.front_case('real', L, n, T, xf, GATE_ERR)
        what = 'front mi=%d L=%d n=%d T=%d x_f32=%d xproj(f32)' % (mi, L, n, T, xf)
        got = twice(lambda: _front(fronts, 'real', L).launch(X, n, T, xf), what)
        assert measured(what, values_of(got, F32), xproj) <= 1.0


@pytest.mark.parametrize('mi', [2, 4])
def test_cbhg_front_a_poisoned_window_stays_alone(fronts, mi):
    """NaN features in the middle one of three windows: its xproj is all NaN, the other two are bit-identical to the run
    without it (T one frame into the second tile, so both window ends sit next to a seam and to a foreign window)."""
    import _vc
    poison_gpu_state()
    _vc.set_option('cbhg_front_mi', mi)
    T = Cs.FRONT_T[mi][-3] if mi == 2 else Cs.FRONT_T[mi][-2]
    f = _front(fronts, 'real', 4)
    for xf in (0, 1):
        X = Cs.front_input('real', 3, T, xf)
        clean = twice(lambda: f.launch(X, 3, T, xf), 'front')
        Xn = X.copy()
        Xn[T:2 * T] = np.nan
        got = f.launch(Xn, 3, T, xf).bits()
        assert np.array_equal(got[:T], clean[:T]) and np.array_equal(got[2 * T:], clean[2 * T:])
        assert np.isnan(values_of(got[T:2 * T], F32)).all()


@pytest.mark.parametrize('mi,L,xf', [(2, 1, 1), (4, 4, 0)])
def test_cbhg_front_through_the_host_packing(mi, L, xf):
    """modules._cbhg_front (the host's re-order of conv1d_1's kernel, its coefficient offsets, its pack calls) on a variable
    store holding the real-valued weights, against chain_ref under the derived bound; the folded norms are the host's."""
    import _vc
    import modules
    poison_gpu_state()
    p = dict(Cs.front_weights('real', L))
    n, T = 2, Cs.FRONT_T[mi][-1]
    X = Cs.front_input('real', n, T, xf)
    st = modules.VariableStore('bfloat16')
    x = torch.from_numpy(X.reshape(n, T, R.FEAT)).to(F32 if xf else BF16).cuda()
    args = dict(embed_size=80, num_conv_banks=6, num_highwaynet_blocks=L, dropout_rate=0.4, is_training=False)
    w = {k: v.numpy() for k, v in _oracle_weights(p, L).items()}
    for d, r0 in (('fw', 0), ('bw', 120)):
        s = 'e/CBHG/gru/bidirectional_rnn/%s/gru_cell/' % d
        w[s + 'gates/kernel'][:R.WIDTH], w[s + 'candidate/kernel'][:R.WIDTH] = p['Wx'][r0:r0 + 80].T, p['Wx'][r0 + 80:r0 + 120].T
        w[s + 'gates/bias'], w[s + 'candidate/bias'] = p['bx'][r0:r0 + 80], p['bx'][r0 + 80:r0 + 120]
    with modules.variable_store(st), modules.variable_scope('e'):
        modules.OPTIONS['cbhg_front'] = False
        try:
            modules.prenet_CBHG(x, **args)                                 # creates the variables
        finally:
            modules.OPTIONS['cbhg_front'] = True
        assert set(st.vars) == set(w), set(st.vars) ^ set(w)
        for name, v in w.items():
            st.assign(name, v.astype(np.float32))
        for name, scope, size in (('b', 'e/CBHG/conv1d_banks/bn', 768), ('p1', 'e/CBHG/conv1d_1', 40), ('p2', 'e/CBHG/conv1d_2', 40)):
            s, b = (t.cpu().double().numpy() for t in modules._prep_bn(st, scope, size))
            p[name + 's'], p[name + 'b'] = s, b
        _vc.set_option('cbhg_front_mi', mi)
        assert _lib().vc_cbhg_front_supported(80, 80, 40, 6, 128, L, 40, T)
        xp = modules._cbhg_front(x, 80, 6, L, 'prenet', 'CBHG')[0]
        xp2 = modules._cbhg_front(x, 80, 6, L, 'prenet', 'CBHG')[0]
    torch.cuda.synchronize()
    assert torch.equal(xp.view(torch.int32), xp2.view(torch.int32))
    ref = R.front(X, p, T, bool(xf), GATE_ERR)
    assert measured('front through modules._cbhg_front mi=%d L=%d T=%d x_f32=%d' % (mi, L, T, xf), xp.cpu().double().numpy(), ref) <= 1.0


def test_cbhg_front_refuses_bad_arguments(fronts):
    import _vc
    poison_gpu_state()
    lib, st = _lib(), _st()
    f = _front(fronts, 'exact', 4)
    X = rows_in(np.zeros((16, R.FEAT)), R.FEAT + 8, BF16)
    out = Out(16, 240, 244, F32)
    fields = [n for n, _ in _vc.CbhgFrontDesc._fields_]

    def desc(**kw):
        d = _vc.CbhgFrontDesc()
        for n in fields:
            if n != 'd_pk_highway':
                setattr(d, n, getattr(f.d, n))
        for l in range(4):
            d.d_pk_highway[l] = f.d.d_pk_highway[l]
        d.d_x, d.x_f32, d.ldx, d.n_windows, d.T, d.d_xproj, d.ldp = X.data_ptr(), 0, R.FEAT + 8, 2, 8, out.t.data_ptr(), 244
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    _refused(lib.vc_cbhg_front(None, st), 'NULL descriptor')
    for kw in (dict(n_features=64), dict(prenet_units=64), dict(width=32), dict(n_banks=5), dict(bank_filters=64), dict(n_highway=-1),
               dict(n_highway=5), dict(gru_units=32), dict(T=7), dict(T=0)):
        _refused(lib.vc_cbhg_front(C.byref(desc(**kw)), st), 'unsupported shape')
    for kw in (dict(d_x=None), dict(d_xproj=None), dict(n_windows=0), dict(n_windows=-1), dict(ldx=72), dict(ldp=236)):
        _refused(lib.vc_cbhg_front(C.byref(desc(**kw)), st), 'NULL tensor or bad leading dimension')
    for kw in (dict(ldx=84), dict(x_f32=1, ldx=82), dict(ldp=242), dict(d_x=X.data_ptr() + 8), dict(d_xproj=out.t.data_ptr() + 8)):
        _refused(lib.vc_cbhg_front(C.byref(desc(**kw)), st), 'must be 16-byte aligned')
    for n in ('d_pk_dense1', 'd_pk_dense2', 'd_pk_bank', 'd_pk_proj1', 'd_pk_proj2', 'd_pk_gru', 'd_coef'):
        _refused(lib.vc_cbhg_front(C.byref(desc(**{n: None})), st), 'NULL or misaligned weight pointer')
        _refused(lib.vc_cbhg_front(C.byref(desc(**{n: getattr(f.d, n) + 8})), st), 'NULL or misaligned weight pointer')
    for l in (0, 3):
        for bad in (None, f.d.d_pk_highway[l] + 8):
            d = desc()
            d.d_pk_highway[l] = bad
            _refused(lib.vc_cbhg_front(C.byref(d), st), 'highway layer %d weights NULL or misaligned' % l)
    assert out.untouched()
    ok = (80, 80, 40, 6, 128, 4, 40, 8)
    assert lib.vc_cbhg_front_supported(*ok) and lib.vc_cbhg_front_supported(80, 80, 40, 6, 128, 0, 40, 400)
    for i, v in ((0, 64), (1, 96), (2, 48), (3, 8), (4, 256), (5, 5), (5, -1), (6, 48), (7, 7)):
        bad = list(ok)
        bad[i] = v
        assert not lib.vc_cbhg_front_supported(*bad), bad
    _ok(lib.vc_cbhg_front(C.byref(desc()), st))
