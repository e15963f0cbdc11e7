"""Inputs of tests/test_chain_kernels_{cpu,gpu}.py: weights and activations of vc_prenet_chain, vc_highway_chain and
vc_cbhg_front, plain numpy on top of tests/chain_ref.py.  The CPU file proves what the GPU file relies on: that the exact
cases are exactly representable and see every layout, and that the real-valued cases' derived bounds stay below the flat
tolerance of tests/test_blocks_gpu.py.

Exact cases: small integers (halves and quarters behind a highway gate of exactly 1/2), sparse where a dense matrix
would push a sum off the bf16 grid; highway gates are pinned with a transform bias or weight of 0 or +-2048 (sigmoid = 1/2,
1 or 0 exactly on the device: exp2 of -+2954 is 0 or inf).
Real-valued cases: sparse weights of one size and shifts that dominate, so that a layer passes on about a third of its
input's relative error and the worst-case bound through ten rounding points stays near 1.5 x 2^-7 of the value.  Such a
bound sees a lost weight only in the last layers (tests/test_chain_kernels_cpu.py measures it); layouts are the exact
cases' job."""
import functools

import numpy as np

import chain_ref as R

PRENET_SHAPES = ((64, 256, 128), (80, 512, 256))
PRENET_M = (1, 31, 32, 33, 127, 128, 129, 257)
HIGHWAY_H = (128, 256)
HIGHWAY_LAYERS = (0, 1, 2, 8)
HIGHWAY_M = (1, 127, 128, 129, 300)
FRONT_T = {2: (8, 9, 54, 55, 108, 109), 4: (8, 118, 119, 237)}
FRONT_WINDOWS = (1, 3)
# what each T is listed for: (tile height, T) -> (tiles per window, frames a block stores, what the last tile holds)
FRONT_SEAMS = {(2, 8): (1, 8, 8), (2, 9): (1, 9, 9), (2, 54): (1, 54, 54), (2, 55): (2, 28, 27), (2, 108): (2, 54, 54), (2, 109): (3, 37, 35),
               (4, 8): (1, 8, 8), (4, 118): (1, 118, 118), (4, 119): (2, 60, 59), (4, 237): (3, 79, 79)}
FLAT_BF16 = 3e-2                 # tests/test_blocks_gpu.py: |device - oracle| <= 3e-2 max(1, max |oracle|)
# largest |device - float64| of vc::highway_gate's sigmoid (v_exp_f32 of -x log2 e, v_rcp_f32 of 1 + that) over [-20, 20.25),
# measured by tests/test_chain_kernels_gpu.py::test_highway_gate_alone on an MI355X (9.661e-8, profiles/chain_kernels/README.md);
# that test holds the device to 4 x this value and every derived bound allows the same
GATE_MAX = 9.7e-8
TIE_DOWN, TIE_UP = 1.0 + 2.0 ** -8, 2.0 - 2.0 ** -8          # float32 numbers half way between two bf16: -> 1 and -> 2


def highway_nw(H):
    return 2 * H // 64


def highway_tails(H):
    nw = highway_nw(H)
    return (64, 64 * nw, 64 * (nw + 1), 6 * H)


def _ints(rng, shape, lo, hi):
    return rng.randint(lo, hi + 1, size=shape).astype(np.float64)


def sparse(rng, rows, K, nz, values):
    """[rows, K] with nz non-zeros per row, drawn by values(n)."""
    W = np.zeros((rows, K))
    for r in range(rows):
        c = rng.choice(K, size=min(nz, K), replace=False)
        W[r, c] = values(len(c))
    return W


def _signs(rng, n):
    return rng.choice([-1.0, 1.0], size=n)


def _real(rng, lo, hi):
    return lambda n: R.to_bf16(rng.uniform(lo, hi, n) * _signs(rng, n))


# ------------------------------------------------------------------------------------------ vc_prenet_chain

@functools.lru_cache(maxsize=None)
def prenet_weights(shape, kind):
    """kind 'onehot': dense1 integers in [-7, 7], every one observed singly by a one-hot row; 'ints': dense1 in {-1, 0, 1}
    for rows of several ones; 'real'.  dense2: 16 (real: 8) non-zeros per row, every K slot used by some row."""
    cin, u1, u2 = shape
    rng = np.random.RandomState(cin + {'onehot': 1, 'ints': 2, 'real': 3}[kind])
    if kind == 'real':
        W1 = sparse(rng, u1, cin, 6, _real(rng, 0.05, 0.15))
        W2 = sparse(rng, u2, u1, 8, _real(rng, 0.03, 0.09))
        return W1, R.to_bf16(rng.uniform(0.3, 0.8, u1)).astype(np.float32), W2, rng.uniform(0.3, 0.8, u2).astype(np.float32)
    W1 = _ints(rng, (u1, cin), -7, 7) if kind == 'onehot' else _ints(rng, (u1, cin), -1, 1)
    W2 = sparse(rng, u2, u1, 16, lambda n: _signs(rng, n))
    for c in np.flatnonzero(np.abs(W2).sum(0) == 0):
        W2[rng.randint(u2), c] = 1.0
    assert (np.abs(W2).sum(0) > 0).all(), 'a K slot of dense2 is never used'
    return W1, _ints(rng, u1, 0, 1), W2, _ints(rng, u2, -2, 2)


def prenet_input(shape, kind, M):
    """(X [M, cin], x_f32): 'onehot' rows e_(m mod cin); 'ints' rows of ones at a quarter of the features; 'ties' float32
    one-hot rows whose one is a bf16 tie (even rows round down to 1, odd rows up to 2); 'real'."""
    cin = shape[0]
    rng = np.random.RandomState(M + cin)
    X = np.zeros((M, cin))
    m = np.arange(M)
    if kind == 'onehot':
        X[m, m % cin] = 1.0
    elif kind == 'ties':
        X[m, (m * 7) % cin] = np.where(m % 2 == 0, TIE_DOWN, TIE_UP)
    elif kind == 'ints':
        X = (rng.rand(M, cin) < 0.25).astype(np.float64)
    else:
        X = R.to_bf16(rng.uniform(-1.0, 1.0, (M, cin)))
    return X


PRENET_EXACT = (('onehot', 'onehot', 0), ('onehot', 'onehot', 1), ('ints', 'ints', 0), ('ties', 'onehot', 1))   # input, weights, x_f32


# ------------------------------------------------------------------------------------------ vc_highway_chain

@functools.lru_cache(maxsize=None)
def highway_weights(H, kind):
    """8 layers (a chain of L uses the first L) and a tail of 6H columns (a tail of n_proj uses the first n_proj).
    exact: layer 0 has dense integer dense1 weights in [-3, 3] and dense2 weights in {0, +-2048}, every one observed
    singly by identity rows; layer 1 one signed weight per unit and a transform bias in {0, +-2048}; layers 2.. the same
    with the bias in +-2048 (a gate of 1/2 halves the grid: two such layers leave quarters).  The tail: integers."""
    rng = np.random.RandomState(H + (0 if kind == 'exact' else 1))
    layers = []
    for l in range(8):
        if kind == 'real':
            W1, W2 = sparse(rng, H, H, 4, _real(rng, 0.03, 0.09)), sparse(rng, H, H, 4, _real(rng, 0.1, 0.3))
            b1, b2 = rng.uniform(0.2, 1.0, H), rng.uniform(0.5, 1.5, H)
        elif l == 0:
            W1, W2 = _ints(rng, (H, H), -3, 3), 2048.0 * _ints(rng, (H, H), -1, 1)
            b1, b2 = _ints(rng, H, 0, 1), np.zeros(H)
        else:
            W1, W2 = sparse(rng, H, H, 1, lambda n: _signs(rng, n)), np.zeros((H, H))
            b1 = _ints(rng, H, 0, 1)
            b2 = 2048.0 * (_ints(rng, H, -1, 1) if l == 1 else _signs(rng, H))
        Wp, bp = R.pair(W1, b1, W2, b2)
        layers.append((Wp, bp.astype(np.float32).astype(np.float64)))
    if kind == 'real':
        PW, pb = sparse(rng, 6 * H, H, 4, _real(rng, 0.1, 0.3)), rng.uniform(-0.5, 0.5, 6 * H).astype(np.float32).astype(np.float64)
    else:
        PW, pb = _ints(rng, (6 * H, H), -2, 2), _ints(rng, 6 * H, -3, 3)
    return layers, (PW, pb)


def highway_input(H, kind, M):
    """exact: identity rows when M == H, else four values of 1 or 2 per row; real: uniform in [-1, 1] on the bf16 grid."""
    rng = np.random.RandomState(H + M)
    if kind == 'real':
        return R.to_bf16(rng.uniform(-1.0, 1.0, (M, H)))
    if M == H:
        return np.eye(H)
    return sparse(rng, M, H, 4, lambda n: _ints(rng, n, 1, 2))


@functools.lru_cache(maxsize=None)
def highway_case(H, kind, L, M, gate_err=0.0):
    """(X, Y Tracked, P Tracked over all 6H tail columns, trace)."""
    layers, tail = highway_weights(H, kind)
    X = highway_input(H, kind, M)
    trace = []
    Y, P = R.highway_chain(X, layers[:L], tail, gate_err, trace)
    return X, Y, P, trace


# ------------------------------------------------------------------------------------------ vc_cbhg_front

FRONT_GATES = (0.0, 2048.0, -2048.0)


@functools.lru_cache(maxsize=None)
def front_weights(kind, n_hw):
    """exact: integers, sparse; folded norms with scales of 1 or 2 and integer shifts, all non-zero bank shifts
    among them (a frame outside the window that is not zeroed then carries relu(shift) > 0 into the pool); conv1d_1's
    matrix has non-zeros in every (width, 32-channel slice, tap, 16-channel half) group; highway gates pinned per unit at
    1/2, 1 or 0."""
    rng = np.random.RandomState(17 + n_hw + (0 if kind == 'exact' else 100))
    C, NB = R.WIDTH, R.BANKS * R.FILTERS
    p = {}
    if kind == 'exact':
        one = lambda n: _signs(rng, n)
        p['W1'], p['b1'] = sparse(rng, R.UNITS, R.FEAT, 10, one), _ints(rng, R.UNITS, 0, 1)
        p['W2'], p['b2'] = sparse(rng, C, R.UNITS, 2, one), _ints(rng, C, 0, 1)
        p['bank'] = [sparse(rng, R.FILTERS, C * k, max(2, k), one) for k in range(1, R.BANKS + 1)]
        p['bs'], p['bb'] = rng.choice([1.0, 2.0], NB), rng.choice([-2.0, -1.0, 1.0, 2.0], NB)
        P1 = np.zeros((C, 3 * NB))
        for g in range(3 * NB // 16):                     # every 16-column group of conv1d_1's K: two weights
            for _ in range(2):
                P1[rng.randint(C), 16 * g + rng.randint(16)] = rng.choice([-1.0, 1.0])
        p['P1'], p['p1s'], p['p1b'] = P1, rng.choice([1.0, 2.0], C), _ints(rng, C, -12, -5)
        p['P2'], p['p2s'], p['p2b'] = sparse(rng, C, 3 * C, 2, one), rng.choice([1.0, 2.0], C), _ints(rng, C, -2, 2)
        p['hw'] = []
        for l in range(n_hw):
            W1 = sparse(rng, C, C, 1, one)
            b2 = rng.choice(FRONT_GATES, C) if l == 0 else rng.choice(FRONT_GATES[1:], C)
            p['hw'].append(R.pair(W1, _ints(rng, C, 0, 1), np.zeros((C, C)), b2))
        p['Wx'], p['bx'] = _ints(rng, (6 * R.GRU, C), -2, 2), _ints(rng, 6 * R.GRU, -3, 3)
    else:
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        p['W1'], p['b1'] = sparse(rng, R.UNITS, R.FEAT, 6, _real(rng, 0.05, 0.15)), f32(rng.uniform(0.3, 0.8, R.UNITS))
        p['W2'], p['b2'] = sparse(rng, C, R.UNITS, 6, _real(rng, 0.03, 0.09)), f32(rng.uniform(0.3, 0.8, C))
        p['bank'] = [sparse(rng, R.FILTERS, C * k, 4, _real(rng, 0.06, 0.12)) for k in range(1, R.BANKS + 1)]
        p['bs'], p['bb'] = f32(rng.uniform(0.8, 1.2, NB)), f32(rng.uniform(0.3, 0.8, NB))
        P1 = np.zeros((C, 3 * NB))
        for g in range(3 * NB // 16):
            P1[rng.randint(C), 16 * g + rng.randint(16)] = _real(rng, 0.03, 0.06)(1)[0]
        p['P1'], p['p1s'], p['p1b'] = P1, f32(rng.uniform(0.8, 1.2, C)), f32(rng.uniform(0.5, 1.0, C))
        p['P2'], p['p2s'], p['p2b'] = sparse(rng, C, 3 * C, 4, _real(rng, 0.04, 0.08)), f32(rng.uniform(0.8, 1.2, C)), f32(rng.uniform(0.2, 0.5, C))
        p['hw'] = []
        for l in range(n_hw):
            Wp, bp = R.pair(sparse(rng, C, C, 4, _real(rng, 0.03, 0.09)), rng.uniform(0.2, 1.0, C),
                            sparse(rng, C, C, 4, _real(rng, 0.1, 0.3)), rng.uniform(0.5, 1.5, C))
            p['hw'].append((Wp, f32(bp)))
        p['Wx'], p['bx'] = sparse(rng, 6 * R.GRU, C, 4, _real(rng, 0.1, 0.3)), f32(rng.uniform(-0.5, 0.5, 6 * R.GRU))
    return p


def front_input(kind, n_windows, T, x_f32):
    """exact: about eight ones per frame (x_f32: float32 bf16 ties that round to 1 or 2); real: uniform on the bf16 grid (x_f32:
    plain float32 numbers, rounded on load)."""
    rng = np.random.RandomState(1000 * n_windows + T + (500 if x_f32 else 0))
    M = n_windows * T
    if kind == 'real':
        X = rng.uniform(-1.0, 1.0, (M, R.FEAT)).astype(np.float32).astype(np.float64)
        return X if x_f32 else R.to_bf16(X)
    on = rng.rand(M, R.FEAT) < 0.1
    if not x_f32:
        return on.astype(np.float64)
    return np.where(on, np.where(rng.rand(M, R.FEAT) < 0.5, TIE_DOWN, TIE_UP), 0.0)


@functools.lru_cache(maxsize=None)
def front_case(kind, n_hw, n_windows, T, x_f32, gate_err=0.0):
    """(X, xproj Tracked, trace)."""
    p = front_weights(kind, n_hw)
    X = front_input(kind, n_windows, T, x_f32)
    trace = []
    return X, R.front(X, p, T, bool(x_f32), gate_err, trace), trace


# the exact front cases: every listed T at both window counts without highway layers, and the pinned gates at the seam sizes
def front_exact_list(mi):
    out = [(0, n, T, x) for T in FRONT_T[mi] for n in FRONT_WINDOWS for x in (0, 1)]
    out += [(L, 3, T, 0) for L in (1, 4) for T in FRONT_T[mi][-2:]]
    return out


def front_real_list(mi):
    return [(L, n, T, x) for (L, n, x), T in zip(((0, 1, 1), (1, 3, 0), (4, 3, 1), (4, 1, 0)), FRONT_T[mi][-4:])]
