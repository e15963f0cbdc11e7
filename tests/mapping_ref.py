"""The spectral-mapping definitions of include/vc_hip.h ("Spectral mapping") restated in numpy.

float64 is the definition on the float32 inputs; ``dtype=np.float32`` runs the likelihood chains with every intermediate
rounded to float32 in the launches' operation order (a fused multiply-add is formed in float64 and rounded once: the product
of two float32 is exact there) -- the control that says what float32 arithmetic alone costs, against which the derived
bounds of the device tests are checked on the CPU.  prepare, update and mlpg are float64 without contraction on the device
and are restated operation by operation: they are compared bit for bit.

Bounds (u = 2^-24), derived as DESIGN.md section 18 derives the speaker kernels':
  cell      |ll_dev - ll_64| <= delta = (3 D + log2 M + 16) u E, E = |c_m*| + q_abs_m* / 2 of the dominant component, q_abs the
            sum of the ABSOLUTE values of the 3 D terms of the quadratic form (the cross term has either sign): a 3 D-term
            fused sum, the table's roundings and a log-sum-exp.
  frame     the same with D terms (the marginal mixture; speaker_ref.frame_bound).
  E-step    gamma = exp(l_m - ll) carries the errors of l_m and of ll, at most delta each: N is off by at most
            2 delta N, a sum S by 2 delta sum gamma |term| (float64 accumulation adds nothing visible), L by delta per cell.
  map       gamma's relative error g = 2 delta + 108 u (the argument's own rounding, at most 104 u where expf does not
            underflow, and expf's 2 ulp).  P = sum_m gamma / Dv: the table's rounding, the product's and an M-term sum:
            (g + (M + 3) u) P.  E_md = fma(A, x - mu_x, mu_y) is off by at most 3 u Eabs, Eabs = |A (x - mu_x)| + |mu_y|, so
            R is off by at most (g + (M + 6) u) sum_m gamma Eabs / Dv and mmse by (g + (M + 5) u) sum_m gamma Eabs.
Nothing here is fitted to a device result."""
import numpy as np

import diff_ref
import mcd_ref
import speaker_ref

U = 2.0 ** -24
W_FLOOR = 2.0 ** -40
TWO_PI = 6.283185307179586476925
TWO_PI_SQ = 39.478417604357434475
TILE = 32
PARTS = 128
CHUNK = 64
FIELDS = ('w', 'mu_x', 'mu_y', 'var_x', 'var_y', 'cov_xy')


def fma32(a, b, c):
    """fmaf on float32 operands: the product of two float32 is exact in float64; the sum with c is rounded to float64 and
    then to float32 (double rounding could differ from the fused result only on a tie of measure zero)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- model
def random_model(M, D, seed=0, spread=1.0):
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.5, 1.5, M)
    vx, vy = rng.uniform(0.2, 2.0, (M, D)), rng.uniform(0.2, 2.0, (M, D))
    rho = rng.uniform(-0.9, 0.9, (M, D))
    mx = spread * rng.standard_normal((M, D))
    my = mx * rng.uniform(0.5, 1.5, (M, D)) + 0.3 * rng.standard_normal((M, D))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(w=f(w / w.sum()), mu_x=f(mx), mu_y=f(my), var_x=f(vx), var_y=f(vy), cov_xy=f(rho * np.sqrt(vx * vy)))


def prepare(model):
    """The table of vc_jd_prepare_f32 as a dict of float32 arrays [M, D] / [M] (not transposed), each the float64 expression
    of the header rounded once; c and cx use numpy's log (the device's may differ in the last float64 bits)."""
    m = {k: np.asarray(model[k], np.float32).astype(np.float64) for k in FIELDS}
    sxx, syy, sxy = m['var_x'], m['var_y'], m['cov_xy']
    det = sxx * syy - sxy * sxy
    M, D = sxx.shape
    acc_c, acc_x = np.zeros(M), np.zeros(M)
    for d in range(D):
        acc_c = acc_c + np.log(TWO_PI_SQ * det[:, d])
        acc_x = acc_x + np.log(TWO_PI * sxx[:, d])
    f = lambda a: a.astype(np.float32)
    return dict(mu_x=f(m['mu_x']), mu_y=f(m['mu_y']), a=f(syy / det), b=f(sxy / det), g=f(sxx / det), ivx=f(1.0 / sxx),
                c=f(np.log(m['w']) - 0.5 * acc_c), cx=f(np.log(m['w']) - 0.5 * acc_x), A=f(sxy / sxx),
                iDv=f(1.0 / (syy - sxy * sxy / sxx)), c64=np.log(m['w']) - 0.5 * acc_c, cx64=np.log(m['w']) - 0.5 * acc_x)


def table_layout(T):
    """The flat table as the launch writes it: six arrays [d][m], c, cx, four arrays [m][d]."""
    tr = [T[k].T.reshape(-1) for k in ('mu_x', 'mu_y', 'a', 'b', 'g', 'ivx')]
    return np.concatenate(tr + [T['c'], T['cx']] + [T[k].reshape(-1) for k in ('mu_x', 'mu_y', 'A', 'iDv')]).astype(np.float32)


def table_floats(M, D):
    return 10 * M * D + 2 * M


def workspace_size(M, D):
    return (PARTS * ((M + CHUNK - 1) // CHUNK) * (CHUNK * (1 + 5 * D) + 2) * 8 + 255) // 256 * 256


def mlpg_workspace_size(B, F, n):
    return (B * F * 5 * n * 8 + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------------------- likelihoods
def joint_loglik(x, y, model, dtype=np.float64, T=None):
    """l [n, M] of the joint density at the pairs (x, y) [n, D], and q_abs [n, M] (float64).  float64: from the model's own
    parameters; float32: from the float32 table, three fused multiply-adds per dimension as the launch has them."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    n, D = x.shape
    if dtype == np.float32:
        T = prepare(model) if T is None else T
        q = np.zeros((n, T['c'].shape[0]), np.float32)
        for d in range(D):
            dx = (x[:, d, None] - T['mu_x'][None, :, d]).astype(np.float32)
            dy = (y[:, d, None] - T['mu_y'][None, :, d]).astype(np.float32)
            q = fma32((T['a'][None, :, d] * dx).astype(np.float32), dx, q)
            q = fma32(((np.float32(-2) * T['b'][None, :, d]) * dx).astype(np.float32), dy, q)
            q = fma32((T['g'][None, :, d] * dy).astype(np.float32), dy, q)
        return fma32(np.float32(-0.5) + 0 * q, q, T['c'][None] + 0 * q), None
    m = {k: np.asarray(model[k], np.float32).astype(np.float64) for k in FIELDS}
    det = m['var_x'] * m['var_y'] - m['cov_xy'] ** 2
    a, b, g = m['var_y'] / det, m['cov_xy'] / det, m['var_x'] / det
    c = np.log(m['w']) - 0.5 * np.log(TWO_PI_SQ * det).sum(1)
    dx = x[:, None, :].astype(np.float64) - m['mu_x'][None]
    dy = y[:, None, :].astype(np.float64) - m['mu_y'][None]
    q = (a * dx * dx - 2.0 * b * dx * dy + g * dy * dy).sum(2)
    q_abs = (np.abs(a) * dx * dx + 2.0 * np.abs(b * dx * dy) + np.abs(g) * dy * dy).sum(2)
    return c[None] - 0.5 * q, q_abs


def marginal_loglik(x, model, dtype=np.float64):
    """l [n, M] of the marginal x-mixture, in speaker_ref's form (the launch's is vc_gmm_loglik_f32's), and q."""
    return speaker_ref.component_loglik(x, model['w'], model['mu_x'], model['var_x'], dtype)


def logsumexp(l, dtype=np.float64):
    l = np.asarray(l, dtype)
    mx = l.max(1)
    return (mx + np.log(np.exp((l - mx[:, None]).astype(dtype)).astype(dtype).sum(1, dtype=dtype)).astype(dtype)).astype(dtype)


def cell_bound(D, M, E):
    return (3.0 * D + np.log2(M) + 16.0) * U * np.asarray(E, np.float64)


def joint_ll(x, y, model, dtype=np.float64):
    """(ll [n], E [n], l [n, M]): E from the float64 run whatever dtype is."""
    l64, q_abs = joint_loglik(x, y, model)
    top = l64.argmax(1)
    m = {k: np.asarray(model[k], np.float64) for k in FIELDS}
    c = np.log(m['w']) - 0.5 * np.log(TWO_PI_SQ * (m['var_x'] * m['var_y'] - m['cov_xy'] ** 2)).sum(1)
    E = np.abs(c[top]) + 0.5 * q_abs[np.arange(len(top)), top]
    l = l64 if dtype == np.float64 else joint_loglik(x, y, model, np.float32)[0]
    return logsumexp(l, dtype), E, l


# ------------------------------------------------------------------------------------------------------------------ E-step
def cells(len_a, len_b, path=None, path_len=None, max_a=None, max_b=None):
    """[n, 2] int64: the cells the launch keeps for one pair, in path order."""
    la = min(max(int(len_a), 0), max_a) if max_a is not None else int(len_a)
    lb = min(max(int(len_b), 0), max_b) if max_b is not None else int(len_b)
    if path is None:
        p = np.arange(min(la, lb), dtype=np.int64)
        return np.stack([p, p], 1)
    n = min(max(int(path_len), 0), len(path))
    c = np.asarray(path[:n], np.int64).reshape(-1, 2)
    ok = (c[:, 0] >= 0) & (c[:, 0] < la) & (c[:, 1] >= 0) & (c[:, 1] < lb)
    return c[ok]


def gather(fa, fb, lens_a, lens_b, paths=None, path_lens=None):
    """The joint vectors of a batch, concatenated: (x [n, D], y [n, D])."""
    xs, ys = [], []
    for b in range(len(fa)):
        c = cells(lens_a[b], lens_b[b], None if paths is None else paths[b], None if paths is None else path_lens[b],
                  fa.shape[1], fb.shape[1])
        xs.append(np.asarray(fa[b], np.float32)[c[:, 0]])
        ys.append(np.asarray(fb[b], np.float32)[c[:, 1]])
    return np.concatenate(xs), np.concatenate(ys)


def accumulate(x, y, model, dtype=np.float64):
    """The statistics over the joint vectors x, y [n, D]: dict N [M], S [5, M, D], L [2] (float64), the absolute sums A [5, M, D]
    of the S bounds, and delta = the largest cell bound."""
    M, D = np.asarray(model['mu_x']).shape
    if len(x) == 0:
        return dict(N=np.zeros(M), S=np.zeros((5, M, D)), A=np.zeros((5, M, D)), L=np.zeros(2), delta=0.0)
    ll, E, l = joint_ll(x, y, model, dtype)
    gam = np.exp((l - ll[:, None]).astype(dtype)).astype(dtype).astype(np.float64)
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    terms = (x64, y64, x64 * x64, y64 * y64, x64 * y64)
    S = np.stack([gam.T @ t for t in terms])
    A = np.stack([gam.T @ np.abs(t) for t in terms])
    return dict(N=gam.sum(0), S=S, A=A, L=np.array([ll.astype(np.float64).sum(), float(len(x))]),
                delta=float(cell_bound(D, M, E).max()))


# ------------------------------------------------------------------------------------------------------------------ update
def update(N, S, model, floor_x, floor_y, rho_max=0.99, min_count=1.0):
    """vc_jd_update_f32 operation by operation (float64, no contraction), each output rounded once."""
    N, S = np.asarray(N, np.float64), np.asarray(S, np.float64)
    M, D = S.shape[1:]
    tot = 0.0
    for k in range(M):
        tot = tot + N[k]
    with np.errstate(all='ignore'):
        wv = N / tot
        w = np.where(wv > W_FLOOR, wv, W_FLOOR).astype(np.float32)
        n = N[:, None]
        ux, uy = S[0] / n, S[1] / n
        rx, ry = S[2] / n - ux * ux, S[3] / n - uy * uy
        fx, fy = np.asarray(floor_x, np.float32).astype(np.float64)[None], np.asarray(floor_y, np.float32).astype(np.float64)[None]
        vx, vy = np.where(rx > fx, rx, fx), np.where(ry > fy, ry, fy)
        lim = np.float64(np.float32(rho_max)) * np.sqrt(vx * vy)
        cv = S[4] / n - ux * uy
        cv = np.where(cv > lim, lim, cv)
        cv = np.where(cv < -lim, -lim, cv)
    keep = (~(N >= np.float64(np.float32(min_count))) | ~(N > 0.0))[:, None]
    out = dict(w=w)
    for k, v in (('mu_x', ux), ('mu_y', uy), ('var_x', vx), ('var_y', vy), ('cov_xy', cv)):
        out[k] = np.where(keep, np.asarray(model[k], np.float32), v.astype(np.float32)).astype(np.float32)
    return out


def init_cells(M, plen):
    plen = np.asarray(plen, np.int64)
    n = int(plen.sum())
    pos = ((2 * np.arange(M, dtype=np.int64) + 1) * n) // (2 * M)
    ends = np.cumsum(plen)
    b = np.minimum(np.searchsorted(ends, pos, side='right'), len(plen) - 1)
    return b, pos - (ends[b] - plen[b])


def fit(fa, fb, lens_a, lens_b, paths=None, path_lens=None, n_components=32, n_iter=20, var_floor=1e-4, rho_max=0.99, min_count=1.0,
        dtype=np.float64):
    """mapping.fit restated: (model dict of float32 arrays, trace [n_iter] float64).  dtype: that of the likelihood chains."""
    fa, fb = np.asarray(fa, np.float32), np.asarray(fb, np.float32)
    B, M, D = len(fa), int(n_components), fa.shape[2]
    x, y = gather(fa, fb, lens_a, lens_b, paths, path_lens)
    one, zero = np.ones((1, D), np.float32), np.zeros((1, D), np.float32)
    unit = dict(w=np.ones(1, np.float32), mu_x=zero, mu_y=zero, var_x=one, var_y=one, cov_xy=zero)
    st = accumulate(x, y, unit, dtype)
    g = update(st['N'], st['S'], unit, zero[0], zero[0], 0.0, 0.0)
    floor_x = (g['var_x'][0] * np.float32(var_floor)).astype(np.float32)
    floor_y = (g['var_y'][0] * np.float32(var_floor)).astype(np.float32)
    plen = [min(lens_a[b], lens_b[b]) if paths is None else min(max(int(path_lens[b]), 0), paths[b].shape[0]) for b in range(B)]
    bi, pi = init_cells(M, plen)
    mx, my = np.zeros((M, D), np.float32), np.zeros((M, D), np.float32)
    for m in range(M):
        i, j = (pi[m], pi[m]) if paths is None else paths[bi[m]][pi[m]]
        mx[m], my[m] = fa[bi[m], max(int(i), 0)], fb[bi[m], max(int(j), 0)]
    model = dict(w=np.full(M, 1.0 / M, np.float32), mu_x=mx, mu_y=my, var_x=np.repeat(g['var_x'], M, 0), var_y=np.repeat(g['var_y'], M, 0),
                 cov_xy=np.zeros((M, D), np.float32))
    trace = np.zeros(n_iter)
    for it in range(n_iter):
        st = accumulate(x, y, model, dtype)
        trace[it] = st['L'][0] / st['L'][1]
        model = update(st['N'], st['S'], model, floor_x, floor_y, rho_max, min_count)
    return model, trace


# --------------------------------------------------------------------------------------------------------------------- map
def map_stats(x, model, mixture='soft', dtype=np.float64):
    """P, R, mmse [n, D], best [n] for the frames x [n, D], and (float64 only) a dict of bounds and the arg-max margin.
    float32: the launch's chain from the float32 table, m ascending."""
    x = np.asarray(x, np.float32)
    n, D = x.shape
    M = len(model['w'])
    l64, q = marginal_loglik(x, model)
    best64 = l64.argmax(1)
    if dtype == np.float32:
        T = prepare(model)
        qq = np.zeros((n, M), np.float32)
        for d in range(D):
            df = (x[:, d, None] - T['mu_x'][None, :, d]).astype(np.float32)
            qq = fma32((df * df).astype(np.float32), T['ivx'][None, :, d] + 0 * df, qq)
        l = fma32(np.float32(-0.5) + 0 * qq, qq, T['cx'][None] + 0 * qq)
        best = l.argmax(1)
        ll = logsumexp(l, np.float32)
        gam = np.exp((l - ll[:, None]).astype(np.float32)).astype(np.float32)
        if mixture == 'best':
            gam = np.zeros_like(gam)
            gam[np.arange(n), best] = 1.0
        P, R, Em = (np.zeros((n, D), np.float32) for _ in range(3))
        for m in range(M):
            if mixture == 'best' and not gam[:, m].any():
                continue
            e = fma32(T['A'][m][None] + 0 * x, (x - T['mu_x'][m][None]).astype(np.float32), T['mu_y'][m][None] + 0 * x)
            gp = (gam[:, m, None] * T['iDv'][m][None]).astype(np.float32)
            sel = gam[:, m, None] != 0 if mixture == 'best' else np.ones((n, 1), bool)
            P = np.where(sel, (P + gp).astype(np.float32), P)
            R = np.where(sel, fma32(gp, e, R), R)
            Em = np.where(sel, fma32(gam[:, m, None] + 0 * e, e, Em), Em)
        return P, R, Em, best, None
    m = {k: np.asarray(model[k], np.float32).astype(np.float64) for k in FIELDS}
    ll = logsumexp(l64)
    gam = np.exp(l64 - ll[:, None])
    if mixture == 'best':
        gam = np.zeros_like(gam)
        gam[np.arange(n), best64] = 1.0
    A = m['cov_xy'] / m['var_x']
    iDv = 1.0 / (m['var_y'] - m['cov_xy'] ** 2 / m['var_x'])
    x64 = x.astype(np.float64)
    dev = A[None] * (x64[:, None, :] - m['mu_x'][None])
    E = m['mu_y'][None] + dev
    Eabs = np.abs(m['mu_y'])[None] + np.abs(dev)
    P = np.einsum('nm,md->nd', gam, iDv)
    R = np.einsum('nm,md,nmd->nd', gam, iDv, E)
    Em = np.einsum('nm,nmd->nd', gam, E)
    cx = np.log(m['w']) - 0.5 * np.log(TWO_PI * m['var_x']).sum(1)
    Efr = np.abs(cx[best64]) + 0.5 * q[np.arange(n), best64]
    delta = speaker_ref.frame_bound(D, M, Efr) if mixture == 'soft' else np.zeros(n)
    g = (2.0 * delta + 108.0 * U)[:, None]
    srt = np.sort(l64, 1)
    margin = srt[:, -1] - srt[:, -2] if M > 1 else np.full(n, np.inf)
    bounds = dict(P=(g + (M + 3) * U) * P, R=(g + (M + 6) * U) * np.einsum('nm,md,nmd->nd', gam, iDv, Eabs),
                  mmse=(g + (M + 5) * U) * np.einsum('nm,nmd->nd', gam, Eabs), margin=margin,
                  delta_best=speaker_ref.frame_bound(D, M, Efr))
    return P, R, Em, best64, bounds


# -------------------------------------------------------------------------------------------------------------------- mlpg
def delta_weight(t, i, F):
    p1, m1, p2, m2 = min(t + 1, F - 1), max(t - 1, 0), min(t + 2, F - 1), max(t - 2, 0)
    return int(i == p1) - int(i == m1) + 2 * (int(i == p2) - int(i == m2))


def mlpg_system(P, R, F):
    """The dense A [n, F, F] and b [n, F] (float64) of the header's definition for one utterance: P, R [>= F, 2 n]."""
    P, R = np.asarray(P, np.float32).astype(np.float64), np.asarray(R, np.float32).astype(np.float64)
    n = P.shape[1] // 2
    W = np.array([[delta_weight(t, i, F) for i in range(F)] for t in range(F)], np.float64) / 10.0
    A, b = np.zeros((n, F, F)), np.zeros((n, F))
    for j in range(n):
        A[j] = np.diag(P[:F, j]) + W.T @ (P[:F, n + j, None] * W)
        b[j] = R[:F, j] + W.T @ R[:F, n + j]
    return A, b


def mlpg(P, R, length, real=np.float64):
    """vc_mlpg_f32 for one utterance, operation by operation, all dimensions at once: (y [max_frames, n] float32, flag).
    ``real``: the arithmetic's type (float64 is the launch's)."""
    P, R = np.asarray(P, np.float32), np.asarray(R, np.float32)
    maxF, D = P.shape
    n = D // 2
    F = min(max(int(length), 0), maxF)
    r = real
    Ps, Pd, Rs, Rd = (a.astype(r) for a in (P[:, :n], P[:, n:], R[:, :n], R[:, n:]))
    y = np.zeros((maxF, n), np.float32)
    Lrows, u = np.zeros((F, 4, n), r), np.zeros((F, n), r)
    Lr, dg, zz = np.zeros((4, 4, n), r), np.ones((4, n), r), np.zeros((4, n), r)
    bad = np.zeros(n, bool)
    with np.errstate(all='ignore'):
        for i in range(F):
            t_lo, t_hi = max(i - 2, 0), min(i + 2, F - 1)
            arow = []
            for s in range(5):
                k = i - 4 + s
                acc = np.zeros(n, r)
                if k >= 0:
                    for t in range(t_lo, t_hi + 1):
                        wgt = delta_weight(t, i, F) * delta_weight(t, k, F)
                        if wgt:                                        # a term whose integer weight is 0 is left out
                            acc = acc + r(wgt) * Pd[t]
                arow.append(acc / r(100))
            arow[4] = Ps[i] + arow[4]
            racc = np.zeros(n, r)
            for t in range(t_lo, t_hi + 1):
                if delta_weight(t, i, F):
                    racc = racc + r(delta_weight(t, i, F)) * Rd[t]
            bi = Rs[i] + racc / r(10)
            v, Li = [None] * 4, [None] * 4
            for s in range(4):
                acc = arow[s]
                for q in range(s):
                    acc = acc - v[q] * Lr[3 - s][q + 4 - s]
                v[s] = acc
                Li[s] = acc / dg[3 - s]
            di = arow[4]
            for s in range(4):
                di = di - v[s] * Li[s]
            zi = bi
            for s in range(4):
                zi = zi - Li[s] * zz[3 - s]
            bad |= ~(di > 0) | ~(di < np.inf)
            Lrows[i], u[i] = np.stack(Li), zi / di
            Lr = np.concatenate([np.stack(Li)[None], Lr[:3]])
            dg = np.concatenate([di[None], dg[:3]])
            zz = np.concatenate([zi[None], zz[:3]])
        yy = np.zeros((4, n), r)
        for i in range(F - 1, -1, -1):
            acc = u[i]
            for q in range(4):
                k = i + 1 + q
                l = Lrows[k, 3 - q] if k < F else np.zeros(n, r)
                acc = acc - l * yy[q]
            y[i] = acc.astype(np.float32)
            yy = np.concatenate([acc[None], yy[:3]])
        if F:
            y[:F, bad] = (Rs[:F, bad] / Ps[:F, bad]).astype(np.float32)
    return y, int(bad.any())


# -------------------------------------------------------------------------------------------------------------------- gain
def bin_table(fb):
    """mapping.bin_table restated."""
    fb = np.asarray(fb, np.float64)
    n_mels, nb = fb.shape
    peak = fb.argmax(1)
    i0, w = np.zeros(nb, np.int32), np.zeros(nb, np.float32)
    for k in range(nb):
        nz = np.flatnonzero(fb[:, k] > 0)
        if len(nz) == 0:
            nz = np.array([int(np.abs(peak - k).argmin())])
        assert len(nz) <= 2 and (len(nz) == 1 or nz[1] == nz[0] + 1), (k, nz)
        if len(nz) == 2:
            i0[k], w[k] = nz[0], fb[nz[1], k] / (fb[nz[0], k] + fb[nz[1], k])
        elif nz[0] <= n_mels - 2:
            i0[k], w[k] = nz[0], 0.0
        else:
            i0[k], w[k] = n_mels - 2, 1.0
    return i0, w


def cep_gain_s(cy, cx, n_frames, dct, i0, w, alpha, db_scale, max_boost_db, max_cut_db, dtype=np.float64):
    """The clamped exponent s [B, F, nb] in dB (rows at or beyond n_frames: NaN).  float32: the launch's arithmetic, every
    product and sum rounded once, ascending from +0."""
    cy, cx = np.asarray(cy, np.float32), np.asarray(cx, np.float32)
    B, F, n = cy.shape
    dct = np.asarray(dct, np.float32).astype(dtype)
    w = np.asarray(w, np.float32).astype(dtype)
    i0 = np.clip(np.asarray(i0), 0, dct.shape[1] - 2)
    s = np.full((B, F, len(i0)), np.nan, dtype)
    sc = dtype(dtype(np.float32(alpha)) * dtype(np.float32(db_scale)))
    lo, hi = dtype(-np.float32(max_cut_db)), dtype(np.float32(max_boost_db))
    for b in range(B):
        nf = F if n_frames is None else min(max(int(n_frames[b]), 0), F)
        df = (cy[b, :nf].astype(dtype) - cx[b, :nf].astype(dtype)).astype(dtype)
        dm = np.zeros((nf, dct.shape[1]), dtype)
        for i in range(n):
            dm = (dm + (dct[i][None] * df[:, i, None]).astype(dtype)).astype(dtype)
        v = (((dtype(1) - w) * dm[:, i0]).astype(dtype) + (w * dm[:, i0 + 1]).astype(dtype)).astype(dtype)
        s[b, :nf] = np.minimum(np.maximum((sc * v).astype(dtype), lo), hi)
    return s


# ------------------------------------------------------------------------------------------------------------------ corpora
def cepstral_corpus(n_utt=10, n=4, seed=5, noise=0.05, lo=60, hi=90):
    """A seeded cepstral corpus: smooth source trajectories x [F, n] and a continuous piecewise-affine target
    y = A x + C |x| + b + noise (affine on every orthant of x).  Returns lists (x, y) of float32 arrays."""
    rng = np.random.RandomState(seed)
    A = np.eye(n) * rng.uniform(0.6, 1.4, n) + 0.2 * rng.standard_normal((n, n))
    C = 0.5 * rng.standard_normal((n, n))
    b = 0.5 * rng.standard_normal(n)
    xs, ys = [], []
    for _ in range(n_utt):
        F = rng.randint(lo, hi)
        z = rng.standard_normal((F + 16, n))
        k = np.hanning(17)
        x = np.stack([np.convolve(z[:, d], k / np.sqrt((k * k).sum()), 'valid') for d in range(n)], 1)
        y = x @ A.T + np.abs(x) @ C.T + b + noise * rng.standard_normal((F, n))
        xs.append(x.astype(np.float32))
        ys.append(y.astype(np.float32))
    return xs, ys


def batch(seqs, pad=0):
    """A list of [F_i, C] arrays as one zero-padded [B, max F + pad, C] float32 array and the lengths."""
    lens = [len(s) for s in seqs]
    out = np.zeros((len(seqs), max(lens) + pad, seqs[0].shape[1]), np.float32)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out, lens


def features_batch(ceps, lens):
    return np.stack([speaker_ref.features_f32(c, l, None, True, False) for c, l in zip(ceps, lens)])


FORMANTS = (((730.0, 1090.0, 2440.0), (90.0, 110.0, 170.0)), ((270.0, 2290.0, 3010.0), (60.0, 100.0, 150.0)),
            ((300.0, 870.0, 2240.0), (70.0, 100.0, 150.0)), ((530.0, 1840.0, 2480.0), (80.0, 100.0, 160.0)))


def sentence(order, durations, scale=1.0, f0=110.0, sr=16000):
    """Four vowels in ``order`` with the segment ``durations`` (seconds), formants times ``scale``, on one pulse train."""
    parts = []
    for k, dur in zip(order, durations):
        n = int(round(dur * sr))
        parts.append((k, n))
    total = sum(n for _, n in parts)
    e = diff_ref.pulse_train(np.full(total, f0), sr)
    out, at = [], 0
    for k, n in parts:
        fo, bw = FORMANTS[k]
        out.append(diff_ref.vowel(e[at:at + n], [f * scale for f in fo], bw, sr)[:n])
        at += n
    return np.concatenate(out)


def wav_corpus(n_pairs=10, seed=3, scale=1.17, sr=16000):
    """n_pairs parallel sentences of about 1 s: the same vowel order and F0 for both speakers, the target's formants times
    ``scale`` and its own segment durations.  Returns (src list, tgt list) of float32 waveforms."""
    rng = np.random.RandomState(seed)
    src, tgt = [], []
    for _ in range(n_pairs):
        order = rng.permutation(4)
        da, db = rng.uniform(0.18, 0.32, 4), rng.uniform(0.18, 0.32, 4)
        src.append(sentence(order, da, 1.0, sr=sr).astype(np.float32))
        tgt.append(sentence(order, db, scale, sr=sr).astype(np.float32))
    return src, tgt


def wav_batch(ws):
    lens = [len(w) for w in ws]
    out = np.zeros((len(ws), max(lens)), np.float32)
    for b, w in enumerate(ws):
        out[b, :len(w)] = w
    return out, lens


def mcd_db(ca, cb, M_dB_norm_factor=0.01):
    """DTW mel-cepstral distortion in dB of two cepstral sequences (mcd_ref's recurrence, float64)."""
    total, n, _ = mcd_ref.dtw(ca, cb, mcd_ref.default_scale(M_dB_norm_factor), want_path=False)
    return float(total) / n


# ------------------------------------------------------------------------------------------------------ end to end, restated
E2E = dict(n_fit=8, n_held=2, n_coef=24, n_components=8, n_iter=10)


def e2e_restatement(cfg, dct, i0, w, dtype=np.float64, corpus=None, **kw):
    """The whole chain on the wav_corpus in numpy: the oracle's front-end, cepstra, features, DTW, fit on the first n_fit pairs,
    conversion of the held-out sources, their gain and the filtered waveforms re-analysed.  dct: the float32 DCT rows the
    device uses; (i0, w): the gain's table.  dtype: that of the likelihood chains (float32: the twin).  Returns a dict of the
    mean held-out MCD in dB: 'before' (source against target), 'cep' (converted cepstra), 'wav' (filtered waveform)."""
    from oracle import frontend_oracle as fo
    import vocoder_kernels_ref as vr
    p = dict(E2E, **kw)
    src, tgt = corpus if corpus is not None else wav_corpus(p['n_fit'] + p['n_held'])
    fe = dict(sr=cfg['sample_rate'], pre_emphasis=cfg['pre_emphasis'], hop_length=cfg['hop_length'], win_length=cfg['win_length'],
              n_mels=cfg['n_mels'], n_mfcc=cfg['n_mfcc'], n_fft=cfg['n_fft'], window=cfg['window'],
              mfcc_normaleze_first_mfcc=cfg['mfcc_normaleze_first_mfcc'], mfcc_norm_factor=cfg['mfcc_norm_factor'],
              calc_mfcc_derivate=cfg['calc_mfcc_derivate'], M_dB_norm_factor=cfg['M_dB_norm_factor'],
              P_dB_norm_factor=cfg['P_dB_norm_factor'], mean_abs_amp_norm=cfg['mean_abs_amp_norm'], clip_output=cfg['clip_output'])
    dct64 = np.asarray(dct, np.float32).astype(np.float64)
    cep = lambda wv: (np.asarray(fo.calc_MFCC_input(wv, **fe)[1], np.float64) @ dct64.T).astype(np.float32)
    ca, cb = [cep(s) for s in src], [cep(t) for t in tgt]
    nf = p['n_fit']
    A, la = batch(ca[:nf])
    Bm, lb = batch(cb[:nf])
    fa, fb = features_batch(A, la), features_batch(Bm, lb)
    paths = [mcd_ref.dtw(ca[b], cb[b])[2] for b in range(nf)]
    model, trace = fit(fa, fb, la, lb, paths, [len(q) for q in paths], p['n_components'], p['n_iter'], dtype=dtype)
    hop, norm = cfg['hop_length'], cfg['M_dB_norm_factor']
    win = vr.device_window(vr.padded_window(cfg['win_length'], cfg['win_length']))
    out = dict(before=[], cep=[], wav=[], trace=trace, model=model, fit_inputs=(fa, fb, la, lb, paths), corpus=(src, tgt))
    for b in range(nf, nf + p['n_held']):
        F = len(ca[b])
        feat = speaker_ref.features_f32(ca[b], F, None, True, False)
        P, R, _, _, _ = map_stats(feat, model, 'soft', dtype)
        y, flag = mlpg(P, R, F)
        assert flag == 0
        s = cep_gain_s(y[None], ca[b][None], [F], dct, i0, w, 1.0, 1.0 / (2.0 * norm), 20.0, 30.0, dtype)
        G = diff_ref.gain_from_s(s)[0]
        n_use = 1 + len(src[b]) // hop
        yw = diff_ref.stft_filter(src[b].astype(np.float64), G, win, hop, n_use)
        out['before'].append(mcd_db(ca[b], cb[b], norm))
        out['cep'].append(mcd_db(y, cb[b], norm))
        out['wav'].append(mcd_db(cep(yw), cb[b], norm))
    for k in ('before', 'cep', 'wav'):
        out[k] = float(np.mean(out[k]))
    return out
