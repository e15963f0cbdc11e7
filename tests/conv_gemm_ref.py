"""float64 definition of one vc_conv_gemm launch, written from the text of include/vc_hip.h (vc_gemm_desc) alone: plain
numpy / torch on the host, no device code.

A launch is described by a `types.SimpleNamespace` (see `desc()`) holding LOGICAL tensors: X [M, channels] without row
padding, per group the transposed kernel W [N, taps * Cin], R [M, N]; strides matter only where the contract makes them
visible (ldc in the dropout index and in the shape of the returned C).  `conv_gemm()` returns C [M, ldc] as float64 with
NaN in every element the launch must not write, so a comparison of the whole buffer checks placement and values at once.
`abs_product()` returns S[m, n] = sum |A| |B| over the same operands, placed in the same columns, for rounding bounds.
"""
import types

import numpy as np
import torch

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
PLAIN, HIGHWAY = 0, 1


def bf16_round(a):
    """float64 array -> the nearest bfloat16 values (round to nearest even), as float64."""
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def f32_round(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def drop_mask(M, ldc, ncol, seed, keep, c_off=0):
    """Host twin of drop_keep_elem (csrc/vc_gemm.hip): element (m, n) of a group whose first column is c_off has the
    index m * ldc + c_off + n; keep iff (splitmix64(idx + seed * phi) >> 40) < keep * 2^24.  Returns 0/1 float64 [M, ncol]."""
    idx = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ldc) + np.uint64(c_off) + np.arange(ncol, dtype=np.uint64)[None, :])
    with np.errstate(over='ignore'):
        x = idx + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    u = (x >> np.uint64(40)).astype(np.float32)
    return (u < np.float32(keep) * np.float32(16777216.0)).astype(np.float64)


def group(W, taps, pad_l, c_off):
    W = np.asarray(W, dtype=np.float64)
    return types.SimpleNamespace(W=W, taps=int(taps), pad_l=int(pad_l), c_off=int(c_off))


def desc(X, T, N, groups, dtype=F32, mode=PLAIN, Cin=None, pro_scale=None, pro_shift=None, pro_relu=0, pro_pool=0,
         epi_scale=None, epi_shift=None, act=ACT_NONE, R=None, ldc=None, out_f32=0, drop_keep=0.0, drop_seed=0,
         sum_groups=0, epi_pool=0):
    X = np.asarray(X, dtype=np.float64)
    d = types.SimpleNamespace(X=X, M=X.shape[0], T=int(T), Cin=int(X.shape[1] if Cin is None else Cin), N=int(N),
                              groups=list(groups), dtype=dtype, mode=mode, pro_scale=pro_scale, pro_shift=pro_shift,
                              pro_relu=int(pro_relu), pro_pool=int(pro_pool), epi_scale=epi_scale, epi_shift=epi_shift,
                              act=act, R=R, out_f32=int(out_f32), drop_keep=float(drop_keep), drop_seed=int(drop_seed),
                              sum_groups=int(sum_groups), epi_pool=int(epi_pool))
    d.ldc = int(ldc) if ldc is not None else out_width(d)
    return d


def out_width(d):
    """Columns of C the launch writes: [0, out_width)."""
    if d.mode == HIGHWAY:
        return d.Cin
    if d.sum_groups:
        return d.N
    return max(g.c_off for g in d.groups) + d.N


def pool_same(P, T):
    """tf.layers.max_pooling1d(2, 1, 'same') inside every window of T rows: out[t] = max(x[t], x[t+1]), out[T-1] = x[T-1]."""
    M, C = P.shape
    W = P.reshape(M // T, T, C)
    out = W.copy()
    if T > 1:
        a, b = W[:, :-1], W[:, 1:]
        # numpy's maximum propagates NaN from either side; so does any honest comparison of the device's result
        out[:, :-1] = np.maximum(a, b)
    return out.reshape(M, C)


def prologue(X, T, scale, shift, relu, pool):
    """The documented order: affine, then ReLU, then the time max-pool.  Acts on REAL frames only: the zeros of the SAME
    padding are inserted afterwards (toeplitz), so they stay zero whatever the shift."""
    P = np.array(X, dtype=np.float64)
    if scale is not None:
        P = P * np.asarray(scale, dtype=np.float64)[None, :] + np.asarray(shift, dtype=np.float64)[None, :]
    if relu:
        P = np.where(np.isnan(P), P, np.maximum(P, 0.0))
    if pool:
        P = pool_same(P, T)
    return P


def toeplitz(P, T, taps, pad_l):
    """A[m, j * C + c] = P[m + j - pad_l, c] if 0 <= (m mod T) + j - pad_l < T else 0."""
    M, C = P.shape
    A = np.zeros((M, taps * C), dtype=np.float64)
    t = np.arange(M) % T
    for j in range(taps):
        tt = t + j - pad_l
        ok = (tt >= 0) & (tt < T)
        rows = np.nonzero(ok)[0]
        A[rows, j * C:(j + 1) * C] = P[rows + j - pad_l]
    return A


def _matmul(A, Wt):
    """A [M, K] @ Wt [N, K]^T in float64.  Rows of A are independent, so a non-finite row stays in its own output row."""
    with np.errstate(invalid='ignore'):
        return A @ Wt.T


def _group_acc(d, g, absval):
    c0 = g.c_off if d.sum_groups else 0
    P = prologue(d.X[:, c0:c0 + d.Cin], d.T, d.pro_scale, d.pro_shift, d.pro_relu, d.pro_pool)
    A = toeplitz(P, d.T, g.taps, g.pad_l)
    assert g.W.shape == (d.N, g.taps * d.Cin), (g.W.shape, d.N, g.taps, d.Cin)
    return _matmul(np.abs(A), np.abs(g.W)) if absval else _matmul(A, g.W)


def _act(v, act):
    if act == ACT_RELU:
        return np.where(np.isnan(v), v, np.maximum(v, 0.0))
    if act == ACT_SIGMOID:
        with np.errstate(over='ignore'):
            return 1.0 / (1.0 + np.exp(-v))
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def _coef(vec, c_off, N, default):
    if vec is None:
        return np.full(N, default, dtype=np.float64)
    return np.asarray(vec, dtype=np.float64)[c_off:c_off + N]


def _store(d, v):
    return f32_round(v) if (d.out_f32 or d.dtype == F32) else bf16_round(v)


def conv_gemm(d, C0=None, round_out=True, parts=None):
    """C [M, ldc] float64 of the launch `d`; NaN where nothing is written (C0 gives other starting contents; it is
    REQUIRED for sum_groups > 1, whose partial tiles are added to it).  round_out=False keeps the float64 values.
    parts: optional dict that receives 'pre' (scale * acc + shift) and 'S' (sum |A| |B|), both [M, ldc], NaN elsewhere."""
    M, N = d.M, d.N
    C = np.full((M, d.ldc), np.nan) if C0 is None else np.array(C0, dtype=np.float64)
    pre_all = np.full((M, d.ldc), np.nan)
    S_all = np.full((M, d.ldc), np.nan)
    rnd = (lambda v: _store(d, v)) if round_out else (lambda v: v)
    if d.mode == HIGHWAY:
        g = d.groups[0]
        H = d.Cin
        acc = _group_acc(d, g, False) + _coef(d.epi_shift, 0, N, 0.0)[None, :]
        S = _group_acc(d, g, True)
        h = np.arange(H)
        colH = 64 * (h // 32) + h % 32          # 32 columns of dense1, then 32 of dense2, per 32 output units
        hp, tp = acc[:, colH], acc[:, colH + 32]
        with np.errstate(over='ignore'):
            sg = 1.0 / (1.0 + np.exp(-tp))
        x = d.X[:, :H]
        C[:, :H] = rnd(np.maximum(hp, 0.0) * sg + x * (1.0 - sg))
        if parts is not None:
            parts.update(hpre=hp, tpre=tp, S_h=S[:, colH], S_t=S[:, colH + 32])
        return C
    if d.sum_groups:
        acc = sum(_group_acc(d, g, False) for g in d.groups)
        S = sum(_group_acc(d, g, True) for g in d.groups)
        if d.sum_groups > 1:
            assert C0 is not None, 'sum_groups > 1 adds to the contents of C'
            C[:, :N] = rnd(C[:, :N] + acc)
            S_all[:, :N] = S
            pre_all[:, :N] = acc
        jobs = [] if d.sum_groups > 1 else [(0, acc, S)]
    else:
        jobs = [(g.c_off, _group_acc(d, g, False), _group_acc(d, g, True) if parts is not None else None) for g in d.groups]
    for c_off, acc, S in jobs:
        s, b = _coef(d.epi_scale, c_off, N, 1.0), _coef(d.epi_shift, c_off, N, 0.0)
        pre = acc * s[None, :] + b[None, :]
        v = _act(pre, d.act)
        if d.drop_keep > 0.0:
            keep = float(np.float32(d.drop_keep))
            v = np.where(drop_mask(M, d.ldc, N, d.drop_seed, d.drop_keep, c_off) != 0.0, v / keep, 0.0)
            if round_out:
                v = f32_round(v)                # the division is a float32 operation of its own
        if d.R is not None:
            v = v + np.asarray(d.R, dtype=np.float64)
        if d.epi_pool:
            v = pool_same(v, d.T)
        C[:, c_off:c_off + N] = rnd(v)
        pre_all[:, c_off:c_off + N] = pre
        if S is not None:
            S_all[:, c_off:c_off + N] = S
    if parts is not None:
        parts.update(pre=pre_all, S=S_all)
    return C


def abs_product(d):
    """S [M, ldc]: sum over k of |A[m, k]| |B[n, k]| for every output element, NaN where nothing is written."""
    if d.mode == HIGHWAY:
        raise ValueError('highway: take S_h / S_t from conv_gemm(parts=...)')
    parts = {}
    C0 = np.zeros((d.M, d.ldc)) if d.sum_groups > 1 else None
    conv_gemm(d, C0=C0, round_out=False, parts=parts)
    return parts['S']


def highway_pack(W1, b1, W2, b2):
    """dense1 / dense2 kernels [H, H] (input, output) and biases [H] -> Bt [64 * ceil(H / 32), H] and the shift vector in
    the interleaved layout of VC_GEMM_HIGHWAY: per 32 output units, 32 rows of dense1^T then 32 rows of dense2^T."""
    H = W1.shape[0]
    NP = 64 * ((H + 31) // 32)
    Bt = np.zeros((NP, H))
    sh = np.zeros(NP)
    h = np.arange(H)
    col = 64 * (h // 32) + h % 32
    Bt[col] = np.asarray(W1, dtype=np.float64).T
    Bt[col + 32] = np.asarray(W2, dtype=np.float64).T
    sh[col], sh[col + 32] = b1, b2
    return Bt, sh
