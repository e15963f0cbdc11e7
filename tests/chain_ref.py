"""Float64 definitions of the fused chain launches (csrc/vc_cbhg_small.hip: vc_cbhg_front, vc_prenet_chain, vc_mfma_pack;
csrc/vc_highway.hip: vc_highway_chain, vc_highway_pack; contracts in include/vc_hip.h), plain numpy, nothing imported from
the package.

  to_bf16          float32 -> bf16, round to nearest even, returned as float64 numbers on the bf16 grid
  prenet           relu(relu(x W1^T + b1) W2^T + b2), rounded to bf16 behind each layer
  front            the encoder's pre-recurrence chain: prenet -> banks k = 1..6 (TF SAME: left (k-1)//2, right k//2;
                   folded scale / shift, relu) -> max_pool(2, 1, same) (the last frame pools with itself) -> conv k = 3 +
                   scale / shift + relu -> conv k = 3 + scale / shift + prenet output -> highway x L -> 40 -> 240
                   projection.  bf16 roundings at dense1, dense2, bank, conv1d_1, conv1d_2 + residual (ONE rounding) and
                   each highway layer; xproj stays unrounded
  highway_chain    L highway layers (paired [2H, H] matrix: rows 64q .. 64q+31 dense1 of units 32q .., rows 64q+32 ..
                   dense2), each rounded to bf16, and an optional dense tail on the last activations (unrounded)
  mfma_pack, highway_pack, proj1_reorder, coef_table     the packed layouts as index formulas

Matrices are [out, in] (row = output channel, K contiguous), as the library takes them.  Every function that computes
values returns a Tracked pair: .v the float64 value, .e a bound, per element, on |correct device result - v|:
  float32 accumulation over K terms in any order    2 (K + 4) 2^-24 (sum |w| (|x| + e_x) + |bias|)
  through a linear layer                            sum |w| e_x
  a bf16 rounding point                             2^-8 |v| for the reference's rounding and 2^-8 (|v| + e) for the
                                                    device's: the two round DIFFERENT numbers e apart, so they can land
                                                    on neighbouring grid points even when e is tiny
  relu, max-pool                                    Lipschitz 1 (pool: the larger of the two errors)
  highway gate y = t (h - x) + x                    t e_h + (1 - t) e_x + |h - x| e_t + e_t (e_h + e_x), with
                                                    e_t = e_tpre / 4 + gate_err (the device's exp2 / rcp sigmoid against
                                                    float64, measured: tests/test_chain_kernels_gpu.py GATE_MAX)
`trace`, when given, receives one record per linear layer and rounding point; exactness(trace) proves a case exactly
representable (every value on the bf16 grid before it is rounded, every product a multiple of one power of two q with
sum |w| |x| < 2^24 q, so that every partial sum in every order is a float32 number).
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS32, EPS16 = 2.0 ** -24, 2.0 ** -8

# vc_cbhg_front's shape (the shipped encoder) and its coefficient table (include/vc_hip.h)
FEAT, UNITS, WIDTH, BANKS, FILTERS, GRU = 80, 80, 40, 6, 128, 40
COEF_FLOATS = 3232
COEF_SLOTS = (('b1', 0, 96), ('b2', 96, 64), ('bs', 160, 1024), ('bb', 1184, 1024), ('p1s', 2208, 64), ('p1b', 2272, 64),
              ('p2s', 2336, 64), ('p2b', 2400, 64), ('bx', 2464, 256))
COEF_HW, COEF_HW_STRIDE, MAX_HIGHWAY = 2720, 128, 4


# ------------------------------------------------------------------------------------------ bf16

def to_bf16_bits(x):
    """float32 -> the 16 bits of its bf16 rounding (nearest, ties to even; NaN stays a quiet NaN of the same sign)."""
    b = np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32).astype(np.uint64)
    nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    r = np.where(nan, (b >> 16) | 0x0040, r)
    return r.astype(np.uint16)


def from_bf16_bits(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def to_bf16(x):
    x = np.asarray(x, dtype=F32)
    return from_bf16_bits(to_bf16_bits(x)).reshape(x.shape).astype(F64)


# ------------------------------------------------------------------------------------------ tracked values

class Tracked:
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=F64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=F64)


def acc_eps(K):
    return 2.0 * (K + 4) * EPS32


def _note(trace, **kw):
    if trace is not None:
        trace.append(kw)


def linear(x, W, bias=None, scale=None, shift=None, trace=None, name=''):
    """x W^T + bias, or fma(x W^T, scale, shift): a float32 accumulation on the device."""
    W = np.asarray(W, dtype=F64)
    K = W.shape[1]
    acc = x.v @ W.T
    S = (np.abs(x.v) + x.e) @ np.abs(W).T
    through = x.e @ np.abs(W).T
    if scale is None:
        b = np.zeros(W.shape[0]) if bias is None else np.asarray(bias, dtype=F64)
        v = acc + b[None, :]
        e = through + acc_eps(K) * (S + np.abs(b)[None, :])
    else:
        sc, sh = np.asarray(scale, dtype=F64), np.asarray(shift, dtype=F64)
        v = acc * sc[None, :] + sh[None, :]
        e = np.abs(sc)[None, :] * through + acc_eps(K) * (np.abs(sc)[None, :] * S + np.abs(sh)[None, :])
    _note(trace, kind='linear', name=name, x=x.v, W=W, out=v)
    return Tracked(v, e)


def relu(x):
    return Tracked(np.maximum(x.v, 0.0), x.e)


def rnd(x, on=True, trace=None, name=''):
    """A bf16 rounding point."""
    _note(trace, kind='round', name=name, x=x.v)
    if not on:
        return x
    return Tracked(to_bf16(x.v), x.e + EPS16 * np.abs(x.v) + EPS16 * (np.abs(x.v) + x.e))


def window_taps(a, T, k):
    """[n T, C] -> [n T, k C]: column block j holds frame t - (k-1)//2 + j of the same window, zeros outside it."""
    a = np.asarray(a, dtype=F64)
    n, C = a.shape[0] // T, a.shape[1]
    w = a.reshape(n, T, C)
    pad_l = (k - 1) // 2
    p = np.concatenate([np.zeros((n, pad_l, C)), w, np.zeros((n, k - 1 - pad_l, C))], axis=1)
    return np.concatenate([p[:, j:j + T] for j in range(k)], axis=2).reshape(n * T, k * C)


def conv_same(x, W, k, T, scale, shift, trace=None, name=''):
    """TF SAME convolution of width k per window of T frames; W [out, k C] with K index = tap * C + channel."""
    return linear(Tracked(window_taps(x.v, T, k), window_taps(x.e, T, k)), W, scale=scale, shift=shift, trace=trace, name=name)


def pool_same(x, T):
    """max_pool(2, 1, same): out[t] = max(x[t], x[t + 1]); the window's last frame pools with itself."""
    def nxt(a):
        w = a.reshape(-1, T, a.shape[1])
        return np.concatenate([w[:, 1:], w[:, -1:]], axis=1).reshape(a.shape)
    return Tracked(np.maximum(x.v, nxt(x.v)), np.maximum(x.e, nxt(x.e)))


def sigmoid(v):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-v))


def pair_rows(H):
    """Rows of dense1 / dense2 of unit u in the paired matrix."""
    u = np.arange(H)
    r = 64 * (u // 32) + u % 32
    return r, r + 32


def pair(W1, b1, W2, b2):
    """dense1 / dense2 [H, H] ([out, in]) and biases -> the paired matrix [64 ceil(H / 32), H] and bias vector."""
    H = np.asarray(W1).shape[0]
    n = 64 * ((H + 31) // 32)
    Wp, bp = np.zeros((n, H)), np.zeros(n)
    hr, tr = pair_rows(H)
    Wp[hr], Wp[tr], bp[hr], bp[tr] = W1, W2, b1, b2
    return Wp, bp


def highway_layer(x, Wp, bp, gate_err=0.0, on=True, trace=None, name='highway'):
    """y = t (h - x) + x with h = relu(x W1^T + b1), t = sigmoid(x W2^T + b2); rounded to bf16."""
    Wp, bp = np.asarray(Wp, dtype=F64), np.asarray(bp, dtype=F64)
    hr, tr = pair_rows(x.v.shape[1])
    h = relu(linear(x, Wp[hr], bp[hr], trace=trace, name=name + '.dense1'))
    tp = linear(x, Wp[tr], bp[tr], trace=trace, name=name + '.dense2')
    t = sigmoid(tp.v)
    et = tp.e / 4.0 + gate_err
    v = t * (h.v - x.v) + x.v
    e = t * h.e + (1.0 - t) * x.e + np.abs(h.v - x.v) * et + et * (h.e + x.e) + 3 * EPS32 * (np.abs(v) + np.abs(x.v) + np.abs(h.v))
    return rnd(Tracked(v, e), on, trace, name)


def highway_chain(X, layers, tail=None, gate_err=0.0, trace=None, rounding=True):
    """X [M, H] on the bf16 grid; layers: list of (paired W, paired bias); tail: (PW [n_proj, H], bias) or None.
    Returns (Y Tracked [M, H], P Tracked [M, n_proj] or None)."""
    x = Tracked(X)
    for i, (Wp, bp) in enumerate(layers):
        x = highway_layer(x, Wp, bp, gate_err, rounding, trace, 'highway%d' % i)
    P = None if tail is None else linear(x, tail[0], tail[1], trace=trace, name='tail')
    return x, P


def prenet(X, W1, b1, W2, b2, x_f32=False, trace=None, rounding=True):
    """X [M, cin] (x_f32: float32 numbers, rounded to bf16 on load -- the same rounding on both sides, no error)."""
    x = Tracked(to_bf16(X) if x_f32 else X)
    y1 = rnd(relu(linear(x, W1, b1, trace=trace, name='dense1')), rounding, trace, 'dense1')
    return rnd(relu(linear(y1, W2, b2, trace=trace, name='dense2')), rounding, trace, 'dense2')


def front(X, p, T, x_f32=False, gate_err=0.0, trace=None, taps=None, rounding=True):
    """vc_cbhg_front.  X [n T, 80]; p: W1 [80, 80], b1, W2 [40, 80], b2, bank (6 matrices [128, 40 k]), bs, bb [768], P1
    [40, 3 * 768] (K index = tap * 768 + channel), p1s, p1b, P2 [40, 120], p2s, p2b, hw (list of (paired W [128, 40],
    paired bias [128])), Wx [240, 40], bx.  rounding=False leaves out every bf16 rounding (the
    float64 network, as oracle/model_oracle.py states it).  Returns xproj Tracked [n T, 240]."""
    pre = prenet(X, p['W1'], p['b1'], p['W2'], p['b2'], x_f32, trace, rounding)
    outs = []
    for k in range(1, BANKS + 1):
        c = slice(FILTERS * (k - 1), FILTERS * k)
        outs.append(rnd(relu(conv_same(pre, p['bank'][k - 1], k, T, p['bs'][c], p['bb'][c], trace, 'bank%d' % k)), rounding, trace, 'bank%d' % k))
    bank = Tracked(np.concatenate([o.v for o in outs], axis=1), np.concatenate([o.e for o in outs], axis=1))
    pooled = pool_same(bank, T)
    c1 = rnd(relu(conv_same(pooled, p['P1'], 3, T, p['p1s'], p['p1b'], trace, 'conv1d_1')), rounding, trace, 'conv1d_1')
    c2 = conv_same(c1, p['P2'], 3, T, p['p2s'], p['p2b'], trace, 'conv1d_2')
    v = c2.v + pre.v
    y = rnd(Tracked(v, c2.e + pre.e + 3 * EPS32 * (np.abs(v) + np.abs(pre.v))), rounding, trace, 'conv1d_2+residual')
    for i, (Wp, bp) in enumerate(p['hw']):
        y = highway_layer(y, Wp, bp, gate_err, rounding, trace, 'highway%d' % i)
    if taps is not None:
        taps.update(prenet=pre, bank=bank, pooled=pooled, conv1d_1=c1, highway=y)
    return linear(y, p['Wx'], p['bx'], trace=trace, name='gru_projection')


# ------------------------------------------------------------------------------------------ exactness

def _quantum(a):
    """The largest power of two that divides every non-zero element (1.0 for an all-zero array)."""
    a = np.abs(np.asarray(a, dtype=F64))
    a = a[a != 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)                                   # a = m 2^e, m in [0.5, 1)
    mi = np.round(m * 2.0 ** 53).astype(np.int64)        # exact: 53-bit integers
    tz = np.zeros(mi.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        z = (mi & ((1 << s) - 1)) == 0
        tz += np.where(z, s, 0)
        mi = np.where(z, mi >> s, mi)
    return float(2.0 ** (e - 53 + tz).min())


def exactness(trace):
    """None when every record of the trace is exactly representable, else a description of the first that is not."""
    for r in trace:
        if r['kind'] == 'round':
            x = r['x']
            if not np.array_equal(to_bf16(x), x):
                return '%s: %d values are off the bf16 grid in front of their rounding' % (r['name'], int((to_bf16(x) != x).sum()))
        else:
            q = _quantum(r['x']) * _quantum(r['W'])
            S = (np.abs(r['x']) @ np.abs(r['W']).T).max() if r['x'].size else 0.0
            if not S / q < 2.0 ** 24:
                return '%s: sum |w| |x| = %g is not below 2^24 quanta of %g' % (r['name'], S, q)
            out = r['out']
            if not np.array_equal(out.astype(F32).astype(F64), out):
                return '%s: the result with its bias / scale and shift is not a float32 number' % r['name']
    return None


# ------------------------------------------------------------------------------------------ packed layouts

def kmap(i, chained):
    """K slot i = 16 s + 8 h + e of a fragment stream -> the column it holds."""
    i = np.asarray(i)
    if not chained:
        return i
    s, h, e = i >> 4, (i >> 3) & 1, i & 7
    return 32 * (s >> 1) + 8 * (2 * (s & 1) + (e >> 2)) + 4 * h + (e & 3)


def mfma_pack(W, rows, K, chained):
    """vc_mfma_pack: packed[(tile nks + s) 64 + lane][e] = W[32 tile + (lane & 31)][kmap(16 s + 8 (lane >> 5) + e)], zero
    outside W.  W [rows, >= K] -> flat [ntiles nks 512]."""
    W = np.asarray(W)
    ntiles, nks = (rows + 31) // 32, (K + 15) // 16
    tl, s, lane, e = np.meshgrid(np.arange(ntiles), np.arange(nks), np.arange(64), np.arange(8), indexing='ij')
    row = 32 * tl + (lane & 31)
    col = kmap(16 * s + 8 * (lane >> 5) + e, chained)
    ok = (row < rows) & (col < K)
    out = np.where(ok, W[np.where(ok, row, 0), np.where(ok, col, 0)], 0)
    return out.reshape(-1).astype(W.dtype)


def highway_pack(Bt, H):
    """vc_highway_pack: packed[w][s][c][lane][j] = Bt[64 w + 32 c + (lane & 31)][16 s + 8 (lane >> 5) + j]."""
    Bt = np.asarray(Bt)
    w, s, c, lane, j = np.meshgrid(np.arange(Bt.shape[0] // 64), np.arange(H // 16), np.arange(2), np.arange(64), np.arange(8), indexing='ij')
    return Bt[64 * w + 32 * c + (lane & 31), 16 * s + 8 * (lane >> 5) + j].reshape(-1)


def proj1_reorder(P1):
    """conv1d_1's matrix [40, 3 * 768] (K index = tap * 768 + (k-1) * 128 + 32 w + 16 s + j) -> d_pk_proj1's K order:
    column ((((k-1) * 4 + w) * 3 + tap) * 2 + s) * 16 + j."""
    P1 = np.asarray(P1)
    k1, w, tap, s, j = np.meshgrid(np.arange(BANKS), np.arange(4), np.arange(3), np.arange(2), np.arange(16), indexing='ij')
    src = tap * (BANKS * FILTERS) + k1 * FILTERS + 32 * w + 16 * s + j
    return P1[:, src.reshape(-1)]


def coef_table(p):
    """d_coef: every vector zero padded to its slot."""
    co = np.zeros(COEF_FLOATS, dtype=F32)
    for name, off, size in COEF_SLOTS:
        v = np.asarray(p[name], dtype=F32)
        assert v.size <= size
        co[off:off + v.size] = v
    assert len(p['hw']) <= MAX_HIGHWAY
    for l, (_, bp) in enumerate(p['hw']):
        co[COEF_HW + COEF_HW_STRIDE * l:COEF_HW + COEF_HW_STRIDE * l + 128] = np.asarray(bp, dtype=F32)
    return co


def front_packed(p):
    """What vc_cbhg_front takes, as (name, matrix, rows, K, chained) in the order of the descriptor's pointers."""
    return [('d_pk_dense1', p['W1'], UNITS, FEAT, 0), ('d_pk_dense2', p['W2'], WIDTH, UNITS, 1),
            ('d_pk_proj1', proj1_reorder(p['P1']), WIDTH, 3 * BANKS * FILTERS, 0), ('d_pk_proj2', p['P2'], WIDTH, 3 * WIDTH, 0),
            ('d_pk_gru', p['Wx'], 6 * GRU, WIDTH, 1)]


# ------------------------------------------------------------------------------------------ vc_cbhg_front's tiling

def front_tiles(T, mi):
    """(tiles_per_win, TF): a block stores at most 32 mi - 10 frames (54 at mi = 2, 118 at mi = 4)."""
    maxtf = 32 * mi - (2 + (BANKS - 1) // 2) - 6
    tiles = (T + maxtf - 1) // maxtf
    return tiles, (T + tiles - 1) // tiles
